"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the reference's goldens.

Tolerances (fp64): operator K.d rel-L2 < 1e-13; one update given the same f_int bit-exact;
trajectories on beam_coarse inside the fp64 re-association noise envelope, with the stated parity
bar rel-L2 < 1e-10 for steps <= 10 000."""
import numpy as np
import pytest

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import fem_oracle as fo
    return fo


def _serial_solver(mesh, E=1e6, nu=0.3, rho=1.0, fz=0.5, gamma=0.9, alpha=0.5, **kw):
    """Serial problem in the reference's first-touch numbering, built with the product's host code."""
    import synchronization_avoiding_algorithms_amd as saa
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes

    lmd, mu = fs.lame(E, nu)
    layouts, _ = fs.build_layouts(mesh.tets, np.zeros(len(mesh.tets), dtype=int), 1, len(mesh.points),
                                  clamp_nodes(mesh))
    lay = layouts[0]
    lumped, fpre = fs.lumped_mass_and_load(mesh.points, mesh.tets, rho, fz)
    dt = fs.cfl_dt(mesh.points, mesh.tets, E, nu, rho, gamma)
    sol = saa.HipExplicitSolver(mesh.points[lay.nodes], lay.cells_local, lumped[lay.local_dof],
                                fpre[lay.local_dof], lay.dirichlet_dofs, lmd, mu, dt, alpha, **kw)
    return sol, lay, dt, lumped, fpre


def noise_bound(step):
    return {1: 1e-15, 10: 1e-14, 100: 1e-13, 1000: 5e-12, 5000: 5e-11}.get(step, 1e-10)


def test_internal_force_matches_reference_spmv(beam_coarse):
    g = load_golden("serial_setup.npz")
    sol, lay, dt, _, _ = _serial_solver(beam_coarse)
    assert np.array_equal(lay.nodes, g["local_nodes"])
    assert dt == float(g["dt"])
    f = sol.internal_force(g["d_rand"])
    assert rel_l2(f, g["Kd_rand"]) < 1e-13
    # linearity / null space: rigid translation produces no force
    t = np.tile([1.0, -2.0, 0.5], sol.n_nodes)
    assert np.abs(sol.internal_force(t)).max() < 1e-7 * np.abs(g["Kd_rand"]).max()
    sol.close()


def test_cd_update_bit_exact(beam_coarse):
    fo = _oracle()
    g = load_golden("serial_setup.npz")
    sol, lay, dt, _, _ = _serial_solver(beam_coarse)
    sol.set_loads(g["F_rankwise"], g["l_M"])  # the reference's own vectors (row-summed mass)
    rng = np.random.default_rng(3)
    n = sol.n_dof
    f_int = rng.normal(size=(n, 1))
    d0 = rng.normal(size=(n, 1)) * 1e-2
    dn = rng.normal(size=(n, 1)) * 1e-2
    for tn in (0.0, 0.37, 1.0, 2.5):
        want = fo.cd_update(f_int, g["F_rankwise"], g["l_M"], d0, dn, np.float64(dt), tn, 0.5,
                            g["local_dirichlet"])
        got = sol.cd_update(f_int, d0, dn, tn)
        assert np.array_equal(got, want), np.abs(got - want).max()
    sol.close()


def test_serial_trajectory_against_reference(beam_coarse):
    g = load_golden("serial_trajectory.npz")
    sol, lay, dt, _, _ = _serial_solver(beam_coarse)
    done = 0
    for s in (int(v) for v in g["steps"]):
        sol.step(s - done)
        done = s
        d0, dn, tn = sol.get_state()
        err = rel_l2(d0[:, 0], g[f"step_{s}"])
        assert err < noise_bound(s), (s, err)
    assert abs(tn - 10000 * dt) < 1e-9
    sol.close()


@pytest.mark.parametrize("n,block_nodes,threads", [(3, 0, 0), (4, 64, 128), (6, 200, 256), (6, 0, 1024), (7, 500, 512)])
def test_synthetic_beam_against_oracle(n, block_nodes, threads):
    """Multi-block plans (halo nodes, duplicated border elements) on the synthetic cantilever.  The last case has
    8 x 8-node block cross-sections, which pack badly in the plan order: most blocks renumber their nodes (saa_plan.cpp:
    block_lattice_order, with the halo lists re-ordered to match), which
    moves the global numbering and the halo lists of their neighbours along."""
    fo = _oracle()
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(n)
    sol, lay, dt, lumped, fpre = _serial_solver(mesh, block_nodes=block_nodes, threads=threads)
    st = sol.plan_stats()
    if n == 7:
        assert st["n_blocks"] == 23 and st["n_renumbered"] >= 10, st
    if block_nodes:
        assert st["n_blocks"] > 1 and st["n_halo_total"] > 0
    ranks, odt, _, _ = fo.setup_problem(mesh.points, mesh.tets, mesh.triangles, 1,
                                        np.zeros(len(mesh.tets), dtype=int))
    assert odt == dt
    assert np.array_equal(ranks[0].nodes, lay.nodes)
    assert rel_l2(lumped, fo.lumped_mass_and_load(mesh.tets, mesh.points, 1.0, 0.5)[0]) < 1e-14
    rng = np.random.default_rng(n)
    d = rng.uniform(-1e-2, 1e-2, size=(sol.n_dof, 1))
    assert rel_l2(sol.internal_force(d), ranks[0].K.dot(d)) < 1e-13
    # start from a rough state so that every dof moves from step 1 on
    d0 = rng.uniform(-1e-4, 1e-4, size=(sol.n_dof, 1))
    dn = d0 + rng.uniform(-1e-6, 1e-6, size=(sol.n_dof, 1))
    d0[ranks[0].dirichlet] = 0
    dn[ranks[0].dirichlet] = 0
    sol.set_state(d0, dn, 0.25)
    tn, o0, on = 0.25, d0, dn
    for _ in range(200):
        o1 = fo.explicit_step(ranks[0].K, ranks[0].F, ranks[0].dirichlet, tn, dt, o0, on, ranks[0].l_M, 0.5)
        on, o0 = o0, o1
        tn = tn + dt
    sol.step(200)
    g0, gn, gt = sol.get_state()
    assert gt == tn
    assert rel_l2(g0, o0) < 1e-11 and rel_l2(gn, on) < 1e-11
    sol.close()


def test_error_paths(beam_coarse):
    import synchronization_avoiding_algorithms_amd as saa
    from synchronization_avoiding_algorithms_amd._lib import SaaError

    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    ones = np.ones(12)
    with pytest.raises(SaaError):  # degenerate element
        saa.HipExplicitSolver(pts * [1, 1, 0], [[0, 1, 2, 3]], ones, ones, [], 1.0, 1.0, 1e-3, 0.5)
    with pytest.raises(SaaError):  # node id out of range
        saa.HipExplicitSolver(pts, [[0, 1, 2, 4]], ones, ones, [], 1.0, 1.0, 1e-3, 0.5)
    with pytest.raises(SaaError):  # zero mass
        saa.HipExplicitSolver(pts, [[0, 1, 2, 3]], 0 * ones, ones, [], 1.0, 1.0, 1e-3, 0.5)
    sol = saa.HipExplicitSolver(pts, [[0, 1, 2, 3]], ones, ones, [0, 1, 2], 1.0, 1.0, 1e-3, 0.5)
    with pytest.raises(SaaError):
        sol.step_finish()  # nothing in flight
    sol.step(3)
    d0, _, tn = sol.get_state()
    assert not d0[:3].any() and np.isfinite(d0).all() and tn > 0
    sol.close()


def test_reference_style_driver_loop_with_dropin_tools(beam_coarse):
    """The time loop of Data_prepare.py:223-240 written against the drop-in ``Tools`` names."""
    from synchronization_avoiding_algorithms_amd.Tools.commons import Time_integration_displacement, elasticity
    from synchronization_avoiding_algorithms_amd.Tools.Dynamic_solver import parallel_explicit_solver_dis_pre
    from synchronization_avoiding_algorithms_amd.Tools.Mat_construction import Local_assembly_for_stiffness

    g = load_golden("serial_setup.npz")
    traj = load_golden("serial_trajectory.npz")
    E, nu = 1e6, 0.3
    elas = elasticity(E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu)), 1, 0.5, True)
    Points, nodes = beam_coarse.points, g["local_nodes"]
    LocalK = Local_assembly_for_stiffness(nodes, beam_coarse.tets[g["local_elements"]], Points, 1, 4, elas, 0)
    assert rel_l2(LocalK.dot(g["d_rand"]), g["Kd_rand"]) < 1e-13
    d_0, d_n, tn, dt = g["d0"], g["dn"], 0, g["dt"]
    for i in range(100):
        Time = Time_integration_displacement(tn, dt, d_0, d_n)
        d1 = parallel_explicit_solver_dis_pre(LocalK, g["F_rankwise"], Points, nodes, g["local_dirichlet"], Time,
                                              elas, g["l_M"], 0.5, 1, 0, MODEL=False)
        assert d1 is not d_0 and d1.shape == d_0.shape
        d_n, d_0, tn = d_0, d1, tn + dt
        if i + 1 in (1, 10, 100):
            assert rel_l2(d1[:, 0], traj[f"step_{i + 1}"]) < noise_bound(i + 1)


def _scrambled_mesh(n, seed, flip_fraction=0.0):
    """Synthetic beam made 'unstructured': jittered nodes, shuffled node and element numbering, random
    even re-orderings of every tet, and (optionally) some tets with two vertices swapped (negative detJ,
    which the reference keeps signed - Mat_construction.py:93)."""
    from synchronization_avoiding_algorithms_amd.mesh import Mesh, structured_beam

    rng = np.random.default_rng(seed)
    m = structured_beam(n)
    pts = m.points + rng.uniform(-0.15, 0.15, size=m.points.shape) / n
    pts[m.points[:, 0] == 0, 0] = 0.0  # keep the clamp plane
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    tets = inv[m.tets]
    even = np.array([[0, 1, 2, 3], [0, 2, 3, 1], [0, 3, 1, 2], [1, 0, 3, 2], [1, 2, 0, 3], [1, 3, 2, 0],
                     [2, 0, 1, 3], [2, 1, 3, 0], [2, 3, 0, 1], [3, 0, 2, 1], [3, 1, 0, 2], [3, 2, 1, 0]])
    tets = np.take_along_axis(tets, even[rng.integers(0, 12, len(tets))], axis=1)
    tets = tets[rng.permutation(len(tets))]
    flip = rng.random(len(tets)) < flip_fraction
    tets[flip] = tets[flip][:, [0, 1, 3, 2]]
    return Mesh(pts[perm], {"tetra": tets, "triangle": inv[m.triangles]}), flip


@pytest.mark.parametrize("n,block_nodes,flip", [(5, 90, 0.0), (6, 150, 0.0), (5, 120, 0.1)])
def test_unstructured_multiblock_operator_and_steps(n, block_nodes, flip):
    """Shuffled / jittered meshes through multi-block plans (pairs, singles, halo) against the oracle;
    with flipped tets only the operator is compared (negative-volume elements make the dynamics unstable)."""
    fo = _oracle()
    mesh, flipped = _scrambled_mesh(n, seed=n, flip_fraction=flip)
    sol, lay, dt, lumped, fpre = _serial_solver(mesh, block_nodes=block_nodes)
    st = sol.plan_stats()
    assert st["n_blocks"] > 4 and st["n_halo_total"] > 0
    ranks, odt, _, _ = fo.setup_problem(mesh.points, mesh.tets, mesh.triangles, 1,
                                        np.zeros(len(mesh.tets), dtype=int))
    rp = ranks[0]
    assert np.array_equal(rp.nodes, lay.nodes)
    rng = np.random.default_rng(1)
    for _ in range(2):
        d = rng.uniform(-1e-2, 1e-2, size=(sol.n_dof, 1))
        assert rel_l2(sol.internal_force(d), rp.K.dot(d)) < 1e-13
    if flip == 0.0:
        assert odt == dt
        d0 = rng.uniform(-1e-5, 1e-5, size=(sol.n_dof, 1))
        d0[rp.dirichlet] = 0
        sol.set_loads(rp.F, rp.l_M)
        sol.set_state(d0, d0, 0.1)
        tn, o0, on = 0.1, d0, d0
        for _ in range(100):
            o1 = fo.explicit_step(rp.K, rp.F, rp.dirichlet, tn, dt, o0, on, rp.l_M, 0.5)
            on, o0, tn = o0, o1, tn + dt
        sol.step(100)
        g0, gn, gt = sol.get_state()
        assert gt == tn and rel_l2(g0, o0) < 1e-11 and rel_l2(gn, on) < 1e-11
    sol.close()


def test_degenerate_sizes():
    """One element; an isolated node (no element touches it); zero steps."""
    import synchronization_avoiding_algorithms_amd as saa

    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0], [5, 5, 5]])
    ones = np.ones(15)
    f = np.zeros(15)
    f[14] = 2.0  # load on the isolated node: it moves freely, d1 = dt^2 F ramp / m (+ damping terms)
    sol = saa.HipExplicitSolver(pts, [[0, 1, 2, 3]], ones, f, [0, 1, 2], 1.0, 1.0, 1e-2, 0.0)
    sol.step(0)
    sol.set_state(np.zeros(15), np.zeros(15), 0.5)
    sol.step(1)
    d0, _, tn = sol.get_state()
    assert d0[14, 0] == (1e-2 ** 2 * (2.0 * 0.5 - 0.0) + 0 - 0 + 0) / (1.0 + 0.0)
    assert not d0[:14].any() and tn == 0.5 + 1e-2
    sol.close()


def test_per_dof_mass_takes_the_general_path():
    """The reference's lumped mass is the same on a node's three dofs (compact per-node array on the device);
    a caller-supplied per-dof mass must still be honoured."""
    fo = _oracle()
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(3)
    sol, lay, dt, _, _ = _serial_solver(mesh, block_nodes=100)
    ranks, _, _, _ = fo.setup_problem(mesh.points, mesh.tets, mesh.triangles, 1, np.zeros(len(mesh.tets), dtype=int))
    rp = ranks[0]
    rng = np.random.default_rng(5)
    lm = rp.l_M * rng.uniform(0.8, 1.25, size=rp.l_M.shape)  # different on x, y, z
    f_any = rp.F + rng.uniform(-1e-3, 1e-3, size=rp.F.shape)  # not of the (0, v, v) form
    for masses, load in ((lm, f_any), (rp.l_M, rp.F)):  # general paths, then back to the compact ones
        sol.set_loads(load, masses)
        d0 = rng.uniform(-1e-5, 1e-5, size=(sol.n_dof, 1))
        d0[rp.dirichlet] = 0
        sol.set_state(d0, d0, 0.2)
        tn, o0, on = 0.2, d0, d0
        for _ in range(50):
            o1 = fo.explicit_step(rp.K, load, rp.dirichlet, tn, dt, o0, on, masses, 0.5)
            on, o0, tn = o0, o1, tn + dt
        sol.step(50)
        g0, gn, _ = sol.get_state()
        assert rel_l2(g0, o0) < 1e-12 and rel_l2(gn, on) < 1e-12
    sol.close()


@pytest.mark.parametrize("n,block_nodes,threads", [(6, 150, 256), (8, 0, 0)])
def test_resident_kernel_equals_one_launch_per_step(n, block_nodes, threads):
    """The resident multi-step kernel (cooperative launches, block image kept in LDS, stamped halo entries) against
    the fused kernel launched once per step: same arithmetic, so only the order of the LDS atomics differs.  Mixed
    call lengths exercise the buffer rotation between the two paths and the 1000-step launch chunks."""
    import torch
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(n)
    calls = (1, 9, 2, 1001, 8, 1, 64)
    fused, _, _, _, _ = _serial_solver(mesh, block_nodes=block_nodes, threads=threads)
    fused.set_resident_kernel(False)
    assert not fused.resident_kernel_info()["capable"]
    resident, lay, _, _, _ = _serial_solver(mesh, block_nodes=block_nodes, threads=threads)
    info = resident.resident_kernel_info()
    assert info["capable"] and info["steps_per_launch"] == 1000 and info["lds_bytes"] <= 160 * 1024
    assert resident.plan_stats()["n_blocks"] > 1  # halo entries do travel between workgroups
    for k in calls:
        fused.step(k)
        resident.step(k)
        a0, an, ta = fused.get_state()
        b0, bn, tb = resident.get_state()
        assert ta == tb
        assert rel_l2(b0, a0) < 1e-12 and rel_l2(bn, an) < 1e-12, k
    # predicted phase (Online_predictor.py:298-301) through the resident kernel: declared-shared nodes take the
    # table rows and are recorded; everything else keeps stepping
    fused.close()
    resident.close()
    shared = np.arange(5, 5 + 12, dtype=np.int32)
    kw = dict(block_nodes=block_nodes, threads=threads, shared_local=shared, shared_slots=np.arange(12, dtype=np.int32),
              n_global_shared=12)
    fused, _, _, _, _ = _serial_solver(mesh, **kw)
    fused.set_resident_kernel(False)
    resident, _, _, _, _ = _serial_solver(mesh, **kw)
    table = (torch.arange(40 * 36, dtype=torch.float64, device="cuda").reshape(40, 36) - 700.0) * 1e-9
    h1 = torch.zeros((50, 36), dtype=torch.float64, device="cuda")
    h2 = torch.zeros_like(h1)
    for sol, h in ((fused, h1), (resident, h2)):
        sol.step(20)
        sol.step_predicted(25, table, 3, h, 10)
        sol.step(9)
    torch.cuda.synchronize()
    assert torch.equal(h1, h2) and torch.equal(h2[10:35], table[3:28])
    assert rel_l2(resident.get_state()[0], fused.get_state()[0]) < 1e-12
    fused.close()
    resident.close()


def test_peer_exchange_inside_the_resident_kernel():
    """saa_step_peer through the resident kernel against saa_step_peer with one launch per step, on one process:
    the loop-back attach (saa_peer_attach_loopback) lets every shared node have two imaginary co-holders living in this rank's own
    inbox (tools/peer_loopback.py), so pushes, stamps, parity double-buffering and rank-ordered sums all run."""
    import torch
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(6)
    shared = np.unique(np.random.default_rng(5).integers(0, len(mesh.points), size=60)).astype(np.int32)
    kw = dict(block_nodes=150, threads=256, shared_local=shared, shared_slots=np.arange(len(shared), dtype=np.int32),
              n_global_shared=len(shared))
    out = []
    for resident in (False, True):
        sol, _, _, _, _ = _serial_solver(mesh, **kw)
        sol.set_resident_kernel(resident)
        assert sol.resident_kernel_info()["capable"] == resident
        sol.peer_attach_loopback(3)
        hist = torch.zeros((300, 3 * len(shared)), dtype=torch.float64, device="cuda")
        for k, row in ((3, 0), (40, 3), (1, 43), (101, 44)):
            sol.step_peer(k, hist, row)
        d0, dn, _ = sol.get_state()
        out.append((d0, dn, hist.cpu().numpy()))
        sol.close()
    for a, b in zip(out[0], out[1]):
        assert rel_l2(b, a) < 1e-12
    dof = (3 * shared[:, None] + np.arange(3)[None, :]).ravel()
    assert np.array_equal(out[1][2][144], out[1][0][dof, 0])  # last history row = shared dofs of the final state


@pytest.mark.parametrize("save_every", [1, 3])
def test_trajectory_recorder_matches_stepwise_downloads(save_every):
    """``saa_set_recorder``: the ground-truth loop's ``d1_save[:, counter] = d1`` (Data_prepare.py:236-240) written by
    the step kernels (fused per-step launches and the resident kernel alike) against downloading the state after
    every step."""
    import torch
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(5)
    n_steps = 150
    ref, _, _, _, _ = _serial_solver(mesh, block_nodes=120, threads=256)
    want = np.zeros((ref.n_dof, int(n_steps / save_every)))
    col = 0
    for i in range(n_steps):
        ref.step(1)
        if i % save_every == 0 and col < want.shape[1]:
            want[:, col] = ref.get_state()[0][:, 0]
            col += 1
    ref.close()
    sol, _, _, _, _ = _serial_solver(mesh, block_nodes=120, threads=256)
    traj = torch.zeros(want.shape, dtype=torch.float64, device="cuda")
    sol.set_recorder(traj, save_every, 0)
    for k in (1, 2, 40, 7, 100):  # 150 steps: single launches, short fused runs, resident launches
        sol.step(k)
    sol.synchronize()
    got = traj.cpu().numpy()
    assert np.abs(got[:, -1]).max() > 0
    assert rel_l2(got, want) < 1e-12
    sol.set_recorder(None)
    sol.step(10)  # recorder off: the matrix is left alone
    sol.synchronize()
    assert np.array_equal(traj.cpu().numpy(), got)
    sol.close()


def test_resident_grid_sizing_several_blocks_per_cu_and_oversized_grids(tmp_path):
    """User-forced ``block_nodes`` / ``threads`` put several workgroups of the resident kernel on a CU: the grid is sized
    by the occupancy query clamped with the scalar-register rule and proved by a census launch (every workgroup checks
    in and waits, bounded, for all the others).  Fitting grids run resident and agree with the fused kernel; a grid
    that cannot be co-resident falls back to one launch per step - cleanly, also when the first check is bypassed and
    the census is what finds out (never a stalled step kernel)."""
    import time

    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(10)
    fits, _, _, _, _ = _serial_solver(mesh, block_nodes=60, threads=256)
    st = fits.plan_stats()
    assert st["n_blocks"] >= 512 and fits.resident_kernel_info()["capable"]      # >= 2 blocks on every CU
    fits.step(300)
    a0, an, _ = fits.get_state()
    fits.set_resident_kernel(False)
    fits.set_state(np.zeros(fits.n_dof), np.zeros(fits.n_dof), 0.0)
    fits.step(300)
    b0, bn, _ = fits.get_state()
    assert rel_l2(a0, b0) < 1e-12 and rel_l2(an, bn) < 1e-12 and np.abs(b0).max() > 0
    fits.close()

    mesh = structured_beam(14)  # 76 125 nodes in blocks of 8: ~9500 workgroups, more than the chip can hold at once
    big, _, _, _, _ = _serial_solver(mesh, block_nodes=8, threads=64)
    assert big.plan_stats()["n_blocks"] > 256 * 32 and not big.resident_kernel_info()["capable"]
    big.step(20)
    ref0 = big.get_state()[0]
    big.close()
    # the census itself: only the diagnostic build of the library (-DSAA_DIAGNOSTICS, tools/) lets an over-sized grid past
    # the first check, so this part runs in a child process on that build
    import os
    import subprocess
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from _diag import diag_library_path

    np.save(tmp_path / "ref0.npy", ref0)
    code = (
        "import sys, time, numpy as np\n"
        f"sys.path[:0] = [{os.path.dirname(os.path.abspath(__file__))!r}, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r}]\n"
        "from test_gpu_parity import _serial_solver, rel_l2\n"
        "from synchronization_avoiding_algorithms_amd.mesh import structured_beam\n"
        "t0 = time.time()\n"
        "forced, _, _, _, _ = _serial_solver(structured_beam(14), block_nodes=8, threads=64)\n"
        "assert not forced.resident_kernel_info()['capable']  # the census saw that not everybody was on the chip\n"
        "forced.step(20)\n"
        "forced.synchronize()  # no bounded wait fired: the step kernels never started resident\n"
        "assert time.time() - t0 < 20.0\n"
        f"assert rel_l2(forced.get_state()[0], np.load({str(tmp_path / 'ref0.npy')!r})) < 1e-13\n"
        "forced.close()\n")
    env = dict(os.environ, SAA_LIB_PATH=diag_library_path(), SAA_RESIDENT_TRUST_GRID="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_split_stepping_of_a_multi_round_plan_equals_one_launch_per_step_and_the_oracle():
    """Partitions beyond the resident kernel's capacity run the fused kernel, several rounds of workgroups per step; their
    blocks are then stepped as three sets (left, between, right) on three streams tied by events, so that one set's launch
    boundaries hide under another's work (saa_api.cpp: split_steps).  Same kernel per block, other schedule: the result
    must be the oracle's, and the plain schedule's up to the order of the LDS atomics."""
    fo = _oracle()
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(8)
    sol, lay, dt, lumped, fpre = _serial_solver(mesh, block_nodes=6, threads=64)
    st = sol.plan_stats()
    sol.set_resident_kernel(False)  # (blocks this small would all fit the chip at once: the fused kernel is what is under test)
    assert st["n_blocks"] >= 2048 and not sol.resident_kernel_info()["capable"], st   # the size from which the split is used
    ranks, odt, _, _ = fo.setup_problem(mesh.points, mesh.tets, mesh.triangles, 1, np.zeros(len(mesh.tets), dtype=int))
    rp = ranks[0]
    assert odt == dt
    rng = np.random.default_rng(8)
    d0 = rng.uniform(-1e-4, 1e-4, size=(sol.n_dof, 1))
    dn = d0 + rng.uniform(-1e-6, 1e-6, size=(sol.n_dof, 1))
    d0[rp.dirichlet] = 0
    dn[rp.dirichlet] = 0
    tn, o0, on = 0.25, d0, dn
    for _ in range(61):
        o1 = fo.explicit_step(rp.K, rp.F, rp.dirichlet, tn, dt, o0, on, rp.l_M, 0.5)
        on, o0, tn = o0, o1, tn + dt
    got = {}
    for split in (1, 0):
        sol.set_option("split_stepping", split)
        sol.set_state(d0, dn, 0.25)
        for k in (40, 3, 18):   # (calls of fewer than four steps take the plain schedule: the two must mix)
            sol.step(k)
        g0, gn, gt = sol.get_state()
        assert gt == tn and rel_l2(g0, o0) < 1e-11 and rel_l2(gn, on) < 1e-11, split
        got[split] = g0
    assert rel_l2(got[1], got[0]) < 1e-12
    sol.close()


def test_two_handles_step_resident_on_two_streams_at_once():
    """Two solvers in one process, each with its own stream, each with a resident grid that fills the chip (256 workgroups
    of the 1M-tet beam): their resident launches must not overlap - each would hold a part of the CUs and wait for the
    rest until the bounded waits give up (SAA_E_STATE, trajectory lost).  The library orders the resident launches of a
    device among themselves; both trajectories come out right, and equal to one launch per step."""
    import torch

    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(19)
    a, _, _, _, _ = _serial_solver(mesh)
    b, _, _, _, _ = _serial_solver(mesh)
    assert a.resident_kernel_info()["capable"] and b.resident_kernel_info()["capable"]
    assert a.plan_stats()["n_blocks"] > 128  # two such grids cannot be on the chip together
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    a.set_stream(sa.cuda_stream)
    b.set_stream(sb.cuda_stream)
    for _ in range(3):  # enqueued back to back on two streams, nothing waits on the host
        a.step(200)
        b.step(200)
    a.synchronize()     # raises if a bounded wait inside a resident kernel gave up
    b.synchronize()
    a0, an, ta = a.get_state()
    b0, bn, tb = b.get_state()
    assert ta == tb and np.abs(a0).max() > 0
    assert rel_l2(a0, b0) < 1e-12 and rel_l2(an, bn) < 1e-12
    b.set_resident_kernel(False)
    b.set_state(np.zeros(b.n_dof), np.zeros(b.n_dof), 0.0)
    b.step(600)
    c0, cn, _ = b.get_state()
    assert rel_l2(a0, c0) < 1e-12 and rel_l2(an, cn) < 1e-12
    a.close()
    b.close()


def test_deterministic_mode_is_bit_reproducible_and_equals_the_atomic_path(monkeypatch):
    """``saa_set_deterministic``: the atomic-free two-kernel step sums a node's element forces in a fixed order.  Two
    independent solvers give IDENTICAL bits after 400 steps and for K.d (the LDS-atomic kernels only agree to round-off
    from run to run); against the default kernels and the oracle the usual round-off bounds hold; the predicted-phase
    overwrite and the begin/finish split work in this mode too; the peer path is refused."""
    import torch
    from synchronization_avoiding_algorithms_amd._lib import SaaError
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    fo = _oracle()
    mesh, _ = _scrambled_mesh(5, seed=11)
    rng = np.random.default_rng(4)
    shared = np.arange(7, 19, dtype=np.int32)
    kw = dict(block_nodes=90, shared_local=shared, shared_slots=np.arange(12, dtype=np.int32), n_global_shared=12)
    runs = []
    d = None
    for _ in range(2):
        sol, lay, dt, _, _ = _serial_solver(mesh, **kw)
        sol.set_deterministic(True)
        if d is None:
            d = rng.uniform(-1e-2, 1e-2, size=(sol.n_dof, 1))
        f = sol.internal_force(d)
        sol.step(150)
        table = (torch.arange(30 * 36, dtype=torch.float64, device="cuda").reshape(30, 36) - 500.0) * 1e-9
        hist = torch.zeros((40, 36), dtype=torch.float64, device="cuda")
        sol.step_predicted(20, table, 2, hist, 5)  # Online_predictor.py:298-301 in this mode
        iface = torch.zeros(36, dtype=torch.float64, device="cuda")
        sol.set_interface_buffer(iface)
        sol.step_begin()                          # partial forces of the shared nodes -> interface buffer
        sol.step_finish()
        sol.step(230)
        with pytest.raises(SaaError):
            sol.step_peer(1)
        runs.append((f, sol.get_state()[0], hist.cpu().numpy(), iface.cpu().numpy()))
        sol.close()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)               # bit for bit
    assert np.array_equal(runs[0][2][5:25], ((np.arange(30 * 36).reshape(30, 36) - 500.0) * 1e-9)[2:22])
    # against the LDS-atomic kernels and the oracle
    ranks, odt, _, _ = fo.setup_problem(mesh.points, mesh.tets, mesh.triangles, 1, np.zeros(len(mesh.tets), dtype=int))
    assert rel_l2(runs[0][0], ranks[0].K.dot(d)) < 1e-13
    plain, _, _, _, _ = _serial_solver(mesh, block_nodes=90)
    det, _, _, _, _ = _serial_solver(mesh, block_nodes=90)
    det.set_deterministic(True)
    assert not det.resident_kernel_info()["capable"] or True  # (capability is a property of the plan; steps go the det way)
    plain.step(400)
    det.step(400)
    o0, _, _, _ = fo.run_ground_truth(ranks, odt, 400)
    assert rel_l2(det.get_state()[0], plain.get_state()[0]) < 1e-12
    assert rel_l2(det.get_state()[0], o0[0]) < 1e-11
    det.set_deterministic(False)                  # back to the fused / resident kernels
    det.step(50)
    plain.step(50)
    assert rel_l2(det.get_state()[0], plain.get_state()[0]) < 1e-12
    plain.close()
    det.close()


DET_FIXTURE = "det_steps.npz"


def _det_fixture_case():
    """Mesh, plan size and host-side plan statistics of ``golden/det_steps.npz``."""
    from synchronization_avoiding_algorithms_amd import plan_host_stats

    mesh, _ = _scrambled_mesh(4, seed=11)
    sol, lay, _, _, _ = _serial_solver(mesh, block_nodes=60)
    st = plan_host_stats(mesh.points[lay.nodes], lay.cells_local, 60)
    return sol, lay, st


def _det_fixture_run(sol, lay):
    """Deterministic mode on the fixture's case: K.d of a seeded d, and the state 60 steps after a seeded start."""
    rng = np.random.default_rng(23)
    sol.set_deterministic(True)
    f = sol.internal_force(rng.uniform(-1e-2, 1e-2, size=(sol.n_dof, 1)))
    d0 = rng.uniform(-1e-5, 1e-5, size=(sol.n_dof, 1))
    d0[lay.dirichlet_dofs] = 0
    sol.set_state(d0, d0, 0.1)
    sol.step(60)
    return f, sol.get_state()[0]


def record_det_steps():
    """Writes ``golden/det_steps.npz`` from the library that is loaded: run it on the commit BEFORE a change of the
    deterministic kernels (``python -c "import test_gpu_parity as t; t.record_det_steps()"`` in tests/, on the GPU)."""
    import os

    from conftest import GOLDEN

    sol, lay, _ = _det_fixture_case()
    f, d = _det_fixture_run(sol, lay)
    sol.close()
    np.savez(os.path.join(GOLDEN, DET_FIXTURE), internal_force=f, state_60=d)
    print(f"wrote {DET_FIXTURE}: {os.path.getsize(os.path.join(GOLDEN, DET_FIXTURE))} bytes")


def test_deterministic_mode_reproduces_the_recorded_bits():
    """Deterministic mode promises the same bits from every build, not only from every run: K.d and the state after 60
    steps equal, bit for bit, what the library recorded in ``golden/det_steps.npz`` before ``det_items_kernel`` came to
    share ``item_forces`` with the atomic kernels.  The plan has paired items, single items and idle slots in blocks with
    halo nodes (asserted from the host-side statistics, so that a plan change cannot hollow the comparison out)."""
    sol, lay, st = _det_fixture_case()
    singles = st["n_elem_copies"] - 2 * st["n_pairs"]
    idle = st["n_items"] - st["n_pairs"] - singles
    print(f"det fixture plan: {st['n_blocks']} blocks, {st['n_pairs']} pairs, {singles} singles, {idle} idle, "
          f"{st['n_halo_total']} halo nodes")
    assert st["n_blocks"] > 1 and st["n_halo_total"] > 0
    assert st["n_pairs"] > 0 and singles > 0 and idle > 0
    want = load_golden(DET_FIXTURE)
    f, d = _det_fixture_run(sol, lay)
    sol.close()
    assert f.shape == want["internal_force"].shape and d.shape == want["state_60"].shape
    assert np.array_equal(f, want["internal_force"])
    assert np.array_equal(d, want["state_60"])


def _delaunay_mesh(n_points, seed):
    """A genuinely unstructured mesh: Delaunay tetrahedra of random points in a 4 x 1 x 1 box (plus a lattice on the
    clamp plane x = 0), positively oriented, slivers dropped (volume < 2 % of the cube of the longest edge: their
    1/detJ makes any two fp64 evaluations of K_e disagree)."""
    from scipy.spatial import Delaunay
    from synchronization_avoiding_algorithms_amd.mesh import Mesh

    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, 6)
    wall = np.stack(np.meshgrid([0.0], g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.concatenate([wall, rng.uniform([0.05, 0, 0], [4, 1, 1], size=(n_points, 3))])
    tri = Delaunay(pts)
    tets = tri.simplices.astype(np.int64)
    p = pts[tets]
    e = p[:, 1:] - p[:, :1]
    vol = np.einsum("ij,ij->i", e[:, 0], np.cross(e[:, 1], e[:, 2])) / 6.0
    tets[vol < 0] = tets[vol < 0][:, [0, 1, 3, 2]]
    longest = np.max(np.linalg.norm(p[:, :, None, :] - p[:, None, :, :], axis=-1), axis=(1, 2))
    tets = tets[np.abs(vol) > 0.02 * longest ** 3]
    used = np.unique(tets)
    remap = np.full(len(pts), -1)
    remap[used] = np.arange(len(used))
    hull = tri.convex_hull
    hull = hull[np.all(pts[hull, 0] < 1e-12, axis=1) & np.all(remap[hull] >= 0, axis=1)]
    return Mesh(pts[used], {"tetra": remap[tets], "triangle": remap[hull]})


@pytest.mark.parametrize("n_points,block_nodes", [(1500, 0), (6000, 200)])
def test_delaunay_mesh_operator_and_steps(n_points, block_nodes):
    """Irregular connectivity (valences 4...40, elements that pair up only partly, ragged blocks): K.d and 60 steps
    against the oracle's assembled matrix, fused and resident kernels."""
    fo = _oracle()
    mesh = _delaunay_mesh(n_points, seed=n_points)
    sol, lay, dt, lumped, fpre = _serial_solver(mesh, block_nodes=block_nodes)
    ranks, odt, _, _ = fo.setup_problem(mesh.points, mesh.tets, mesh.triangles, 1, np.zeros(len(mesh.tets), dtype=int))
    rp = ranks[0]
    assert odt == dt and np.array_equal(rp.nodes, lay.nodes) and len(rp.dirichlet) >= 3 * 30
    st = sol.plan_stats()
    assert st["n_elem_copies"] >= len(mesh.tets)
    rng = np.random.default_rng(1)
    d = rng.uniform(-1e-3, 1e-3, size=(sol.n_dof, 1))
    assert rel_l2(sol.internal_force(d), rp.K.dot(d)) < 1e-12
    sol.set_loads(rp.F, rp.l_M)
    d0 = rng.uniform(-1e-6, 1e-6, size=(sol.n_dof, 1))
    d0[rp.dirichlet] = 0
    tn, o0, on = 0.3, d0, d0
    for _ in range(60):
        o1 = fo.explicit_step(rp.K, rp.F, rp.dirichlet, tn, dt, o0, on, rp.l_M, 0.5)
        on, o0, tn = o0, o1, tn + dt
    for resident in (True, False):
        sol.set_resident_kernel(resident)
        sol.set_state(d0, d0, 0.3)
        sol.step(60)
        g0, gn, gt = sol.get_state()
        assert gt == tn and rel_l2(g0, o0) < 1e-10 and rel_l2(gn, on) < 1e-10, resident
    sol.close()
