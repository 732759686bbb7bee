"""The step kernels (csrc/saa_kernels.hip: fused, resident, deterministic) against the CPU oracle at the shapes of
step_edges.py - the far and the near side of every per-thread sweep depth, no halo at all, workgroups that are not a power
of two, the resident kernel's LDS limit from both sides - and the resident kernel across its launch boundaries and the
two counter wraps.  test_step_edge_shapes.py proves (without a GPU) that every shape reaches the regime in its name and
that a single stale read in the oracle moves the result by >= 100 x the bar used here.

Bars: those of test_gpu_parity.py (operator 1e-13, 200 steps 1e-11; Delaunay 1e-12 / 1e-10; resident against fused 1e-12;
long runs ``noise_bound``).  Every figure is printed before it is asserted (``pytest -s`` shows them).

Measured on an MI355X when these tests were written (worst over the shapes and paths): K.d 7.5e-16 (Delaunay 3.6e-16);
200 steps against the oracle 2.3e-13 (Delaunay 1.4e-14); resident against fused 2.2e-13 after 8022 steps, 5.3e-14 through
the peer exchange; 192, 320, 704 and 960 threads all passed the census and ran resident; block_nodes 1100 / 1200 on
structured_beam(8) give a resident image of 161 360 bytes (2480 under the limit) / 171 768 bytes (refused).  Hand-made
mutants of the library that each turn tests of this file red while test_gpu_parity.py stays green: the resident kernel's
halo tail skipping its last dof (deep shapes); ``table_row0`` not advancing from launch to launch (predicted phase across
launches); the resident kernel's tn computed as tn0 + (s + 1) dt (one-wave bit equality); the peer sequence continuing at 1
after 0xffffffff (parity counter of the wrap test)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import step_edges as se
from conftest import REPO, rel_l2
from test_gpu_parity import _serial_solver

pytestmark = pytest.mark.gpu

WAIT_S = 5.0  # bound of every in-kernel wait in these tests: a mistake shows as SAA_E_STATE at once, not as a long wait


def _oracle():
    from oracle import fem_oracle as fo
    return fo


def _solver(shape, mesh, **kw):
    """The serial solver of a shape of the table (None: the automatic plan) with short bounded waits."""
    if shape is not None:
        kw = dict(block_nodes=shape.block_nodes, threads=shape.threads, **kw)
    sol, lay, dt, _, _ = _serial_solver(mesh, **kw)
    sol.set_option("wait_timeout_s", WAIT_S)
    return sol, lay, dt


def _shared_kw(n_nodes):
    shared = se.spread_nodes(n_nodes)
    return shared, dict(shared_local=shared, shared_slots=np.arange(len(shared), dtype=np.int32), n_global_shared=len(shared))


def _dofs(nodes):
    return (3 * np.asarray(nodes)[:, None] + np.arange(3)[None, :]).ravel()


# ---- B. every shape, every stepping path it admits, against the oracle ------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in se.SHAPES])
def test_shape_operator_and_200_steps_on_every_path_against_the_oracle(name):
    shape = se.by_name(name)
    c = se.oracle_case(shape.mesh_id)
    mesh, rp, dt = c["mesh"], c["rp"], c["dt"]
    op_bar, bar = se.bars(shape)
    sol, lay, sdt = _solver(shape, mesh)
    assert sdt == dt and np.array_equal(rp.nodes, lay.nodes)
    _, st_host, mx, threads = se.plan_facts(shape)
    st = sol.plan_stats()
    assert st["threads"] == threads and all(st[k] == st_host[k] for k in ("n_blocks", "max_owned", "max_local", "n_items"))
    info = sol.resident_kernel_info()
    raw, padded = se.resident_lds_bytes(st_host, mx)
    print(f"\n{name}: threads {threads}, resident capable {info['capable']}, lds_bytes {info['lds_bytes']} (formula {raw})")
    if shape.resident is True:
        assert info["capable"] and info["lds_bytes"] == padded <= se.LDS_LIMIT
    elif shape.resident is False:
        assert not info["capable"] and info["lds_bytes"] == 0 and raw > se.LDS_LIMIT
    if "lds_just_under" in shape.regimes:
        assert se.LDS_LIMIT - 8 * 1024 <= info["lds_bytes"] <= se.LDS_LIMIT

    rng = np.random.default_rng(1)
    d = rng.uniform(-1e-2, 1e-2, size=(sol.n_dof, 1)) * (0.1 if shape.delaunay else 1.0)
    e_op = rel_l2(sol.internal_force(d), rp.K.dot(d))
    print(f"{name}: K.d rel-L2 {e_op:.2e} (bar {op_bar:.0e})")
    assert e_op < op_bar
    # (the product's own lumped mass and load stay in place: with the oracle's vectors uploaded - as
    # test_delaunay_mesh_operator_and_steps does - the compact per-node forms are gone and nothing runs resident)

    paths = (["resident"] if info["capable"] else []) + ["fused", "deterministic"]
    for path in paths:
        sol.set_resident_kernel(path == "resident")
        sol.set_deterministic(path == "deterministic")
        assert sol.resident_kernel_info()["capable"] == (path == "resident")
        sol.set_state(c["d0"], c["dn"], se.TN0)
        sol.step(se.N_STEPS)   # returns: every wait in the kernels is bounded by WAIT_S
        sol.synchronize()      # raises SAA_E_STATE if one of them gave up
        g0, gn, gt = sol.get_state()
        e0, en = rel_l2(g0, c["o0"]), rel_l2(gn, c["on"])
        print(f"{name}: {path:13s} {se.N_STEPS} steps rel-L2 d0 {e0:.2e} dn {en:.2e} (bar {bar:.0e}), tn equal {gt == c['tn']}")
        assert gt == c["tn"], (path, gt, c["tn"])
        assert e0 < bar and en < bar, (path, e0, en)
    sol.close()


# ---- B. one-wave workgroups: resident and fused kernels to the same bits ------------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in se.SHAPES if s.threads == 64])
def test_one_wave_workgroups_step_resident_and_fused_to_the_same_bits(name):
    """With 64 threads a workgroup is ONE wave: its LDS atomics execute in program order, and both kernels sweep a block's
    lists in the same order (interior items in sweeps of 64, then the boundary items; the fused kernel's wave-balance shift
    is taken modulo one wave, i.e. 0).  The arithmetic per item and per dof is the same code, so the two paths must agree
    bit for bit - which makes the last bit of everything the resident kernel keeps to itself visible: its own copy of tn
    (hence the load ramp while tn < 1) must be the repeated sum tn + dt the fused path gets from the host, not
    tn0 + s * dt, which differs from it by a few ulp after a hundred steps."""
    shape = se.by_name(name)
    c = se.oracle_case(shape.mesh_id)
    assert c["tn"] < 1.0 and c["tn"] != se.TN0 + se.N_STEPS * c["dt"]  # the ramp is still rising, and the two sums differ
    sol, _, _ = _solver(shape, c["mesh"])
    assert sol.plan_stats()["threads"] == 64 and sol.resident_kernel_info()["capable"]
    out = {}
    for path in ("resident", "fused"):
        sol.set_resident_kernel(path == "resident")
        sol.set_state(c["d0"], c["dn"], se.TN0)
        sol.step(se.N_STEPS)
        out[path] = sol.get_state()
    sol.close()
    diff = rel_l2(out["resident"][0], out["fused"][0])
    print(f"\n{name}: one wave per workgroup, resident against fused after {se.N_STEPS} steps: {diff:.2e} (must be 0)")
    assert np.array_equal(out["resident"][0], out["fused"][0]) and np.array_equal(out["resident"][1], out["fused"][1])
    assert out["resident"][2] == out["fused"][2] == c["tn"]


# ---- B. the deep and the shallow shape with declared shared nodes ---------------------------------------------------------------
@pytest.mark.parametrize("name", se.SHARED_NODE_SHAPES)
def test_shape_with_shared_nodes_predicted_phase_and_peer_exchange(name):
    import torch

    fo = _oracle()
    shape = se.by_name(name)
    c = se.oracle_case(shape.mesh_id)
    mesh, rp, dt = c["mesh"], c["rp"], c["dt"]
    shared, kw = _shared_kw(len(rp.nodes))
    width = 3 * len(shared)
    assert len(shared) == 12
    # predicted phase: table rows land in the state and in the history, bit for bit
    table = (torch.arange(40 * width, dtype=torch.float64, device="cuda").reshape(40, width) - 700.0) * 1e-9
    out = {}
    for path in ("fused", "resident"):
        sol, _, _ = _solver(shape, mesh, **kw)
        sol.set_resident_kernel(path == "resident")
        assert sol.resident_kernel_info()["capable"] == (path == "resident")
        sol.set_state(c["d0"], c["dn"], se.TN0)
        h = torch.full((50, width), -7.0, dtype=torch.float64, device="cuda")
        sol.step(20)
        sol.step_predicted(25, table, 3, h, 10)
        after = sol.get_state()[0]
        sol.step(9)
        sol.synchronize()
        out[path] = (h.cpu().numpy(), after, sol.get_state()[0])
        sol.close()
    t = table.cpu().numpy()
    for path in out:
        h = out[path][0]
        assert np.array_equal(h[10:35], t[3:28]), path
        assert (h[:10] == -7.0).all() and (h[35:] == -7.0).all(), path
        assert np.array_equal(out[path][1][_dofs(shared), 0], t[27]), path  # the shared dofs of the state ARE the last row
    for k in (1, 2):
        e = rel_l2(out["resident"][k], out["fused"][k])
        print(f"\n{name}: predicted phase, resident against fused rel-L2 {e:.2e} (bar 1e-12)")
        assert e < 1e-12

    # loop-back peer exchange with three holders: shared nodes see three times their local force
    n_steps = se.N_STEPS
    sh_dof = _dofs(shared)
    o0, on, tn, hist_ref = se.oracle_steps_loopback(fo, rp, dt, c["d0"], c["dn"], se.TN0, n_steps, sh_dof, 3)
    assert rel_l2(o0, c["o0"]) > 1e-3  # (the tripled force does change the trajectory: the exchange is visible)
    got = {}
    for path in ("fused", "resident"):
        sol, _, _ = _solver(shape, mesh, **kw)
        sol.set_resident_kernel(path == "resident")
        sol.peer_attach_loopback(3)
        sol.set_state(c["d0"], c["dn"], se.TN0)
        hist = torch.zeros((n_steps + 4, width), dtype=torch.float64, device="cuda")
        for k, row in ((3, 0), (n_steps - 4, 3), (1, n_steps - 1)):
            sol.step_peer(k, hist, row)
        sol.synchronize()
        g0, gn, gt = sol.get_state()
        h = hist.cpu().numpy()
        e0, en, eh = rel_l2(g0, o0), rel_l2(gn, on), rel_l2(h[:n_steps], hist_ref)
        print(f"{name}: peer loop-back {path:8s} against the oracle d0 {e0:.2e} dn {en:.2e} history {eh:.2e} (bar 1e-11)")
        assert gt == tn and e0 < 1e-11 and en < 1e-11 and eh < 1e-11, path
        assert np.array_equal(h[n_steps - 1], g0[sh_dof, 0]) and not h[n_steps:].any()
        got[path] = (g0, gn, h)
        sol.close()
    for a, b in zip(got["fused"], got["resident"]):
        e = rel_l2(b, a)
        print(f"{name}: peer loop-back resident against fused {e:.2e} (bar 1e-12)")
        assert e < 1e-12


# ---- C. launch boundaries of the resident kernel ----------------------------------------------------------------------------------
C_MESH = "beam5"
C_CALLS = (1000, 1007, 1008, 2000, 7, 3000)  # one launch; one of 1007; 1000 + 8; two full; one launch per step; three
#                                            (8022 steps in all)
C_EVERY, C_COLS = 7, 500                     # the last column (step index 3493) is written in the middle of a launch


def long_run_bar(steps):
    """The project's stated parity bar for long runs (test_gpu_parity.py: noise_bound - set on the reference mesh from
    rest), and where the rough start of this input needs more: twice what the FUSED kernel - one launch per step, independent
    of everything part C tests - was measured at against the oracle on an MI355X.  Fused kernel against the oracle after
    1000 / 2007 / 3015 / 5015 / 5022 / 8022 steps: 2.4e-12 / 9.5e-12 / 2.1e-11 / 5.3e-11 / 5.3e-11 / 1.25e-10 - inside the
    stated bar (5e-12 / 5e-11 / 5e-11 / 1e-10 / 1e-10) everywhere but at the last point, which gets 2 x 1.25e-10."""
    stated = 5e-12 if steps <= 1000 else 5e-11 if steps <= 5000 else 1e-10
    return max(stated, 2 * C_FUSED_MEASURED.get(steps, 0.0))


C_FUSED_MEASURED = {8022: 1.25e-10}


def _c_problem():
    c = se.oracle_case(C_MESH)
    shared, kw = _shared_kw(len(c["rp"].nodes))
    return c, shared, kw


def test_plain_steps_and_recorder_across_resident_launch_boundaries():
    """8022 steps in calls that are one launch, one launch of 1007, 1000 + 8, two full launches, one launch per step and
    three launches, with a recorder whose last column falls inside a launch: against the same calls through the fused kernel
    (1e-12) and against the oracle (noise_bound of test_gpu_parity.py), tn equal to the oracle's repeated sum."""
    import torch

    fo = _oracle()
    c, shared, kw = _c_problem()
    rp, dt = c["rp"], c["dt"]
    assert sum(C_CALLS) == 8022 and C_COLS < 8022 // C_EVERY
    # oracle: state after every call, and the recorder's columns (column j = the result of step index 7 j)
    want_cols = np.zeros((3 * len(rp.nodes), C_COLS))
    o0, on, tn, done, states = c["d0"], c["dn"], se.TN0, 0, []
    for k in C_CALLS:
        for _ in range(k):
            o1 = fo.explicit_step(rp.K, rp.F, rp.dirichlet, tn, dt, o0, on, rp.l_M, 0.5)
            on, o0, tn = o0, o1, tn + dt
            if done % C_EVERY == 0 and done // C_EVERY < C_COLS:
                want_cols[:, done // C_EVERY] = o0[:, 0]
            done += 1
        states.append((o0, on, tn))
    got = {}
    for path in ("fused", "resident"):
        sol, _, _ = _solver(None, c["mesh"], **kw)
        st = sol.plan_stats()
        assert 32 <= st["n_blocks"] <= 64 and st["n_halo_total"] > 0  # launches of many workgroups that do exchange values
        sol.set_resident_kernel(path == "resident")
        info = sol.resident_kernel_info()
        assert info["capable"] == (path == "resident") and info["steps_per_launch"] == se.RESIDENT_CHUNK
        traj = torch.full((sol.n_dof, C_COLS), -7.0, dtype=torch.float64, device="cuda")
        sol.set_recorder(traj, C_EVERY, 0)
        sol.set_state(c["d0"], c["dn"], se.TN0)
        per_call, total = [], 0
        for k, (w0, wn, wt) in zip(C_CALLS, states):
            sol.step(k)
            total += k
            g0, gn, gt = sol.get_state()
            e0, en = rel_l2(g0, w0), rel_l2(gn, wn)
            print(f"\n{path:8s} after {total:5d} steps: against the oracle d0 {e0:.2e} dn {en:.2e} (bar {long_run_bar(total):.0e}), "
                  f"tn equal {gt == wt}")
            assert gt == wt, (path, total)
            assert e0 < long_run_bar(total) and en < long_run_bar(total), (path, total, e0, en)
            per_call.append((g0, gn))
            if total == 3015:
                before_last_col = traj.cpu().numpy()
                assert (before_last_col[:, 3015 // C_EVERY + 1:] == -7.0).all()  # columns of later steps: still untouched
        sol.synchronize()
        cols = traj.cpu().numpy()
        e = rel_l2(cols, want_cols)
        print(f"{path:8s} recorder, {C_COLS} columns: against the oracle {e:.2e}")
        assert e < long_run_bar(C_EVERY * (C_COLS - 1) + 1) and not (cols == -7.0).any()
        got[path] = (per_call, cols)
        sol.close()
    for (f0, fn), (r0, rn), k in zip(got["fused"][0], got["resident"][0], np.cumsum(C_CALLS)):
        e0, en = rel_l2(r0, f0), rel_l2(rn, fn)
        print(f"resident against fused after {k:5d} steps: d0 {e0:.2e} dn {en:.2e} (bar 1e-12)")
        assert e0 < 1e-12 and en < 1e-12, k
    e = rel_l2(got["resident"][1], got["fused"][1])
    print(f"resident against fused, recorder: {e:.2e} (bar 1e-12)")
    assert e < 1e-12


def test_predicted_phase_across_three_resident_launches():
    """step_predicted(3000, table, 5, hist, 11): every launch must continue in the table and in the history where the one
    before stopped - all entries of the table are distinct, so a repeated or shifted row shows."""
    import torch

    c, shared, kw = _c_problem()
    width = 3 * len(shared)
    table = (torch.arange(3010 * width, dtype=torch.float64, device="cuda").reshape(3010, width) - 50000.0) * 1e-10
    assert torch.unique(table).numel() == table.numel() and float(table.abs().max()) < 1e-4
    out = {}
    for path in ("fused", "resident"):
        sol, _, _ = _solver(None, c["mesh"], **kw)
        sol.set_resident_kernel(path == "resident")
        assert sol.resident_kernel_info()["capable"] == (path == "resident")
        sol.set_state(c["d0"], c["dn"], se.TN0)
        hist = torch.full((3020, width), -7.0, dtype=torch.float64, device="cuda")
        sol.step_predicted(3000, table, 5, hist, 11)
        sol.synchronize()
        g0, gn, _ = sol.get_state()
        out[path] = (g0, gn)
        assert torch.equal(hist[11:3011], table[5:3005]), path
        assert bool((hist[:11] == -7.0).all()) and bool((hist[3011:] == -7.0).all()), path
        assert np.array_equal(g0[_dofs(shared), 0], table[3004].cpu().numpy()), path
        sol.close()
    for a, b in zip(out["fused"], out["resident"]):
        e = rel_l2(b, a)
        print(f"\npredicted phase, 3000 steps: resident against fused {e:.2e} (bar 1e-12)")
        assert e < 1e-12


def test_peer_exchange_across_three_resident_launches():
    """peer_attach_loopback(3) + step_peer(2500, hist, 3): launches of 1000, 1000 and 500 steps; the sequence numbers of the
    exchange and the history rows continue from launch to launch."""
    import torch

    c, shared, kw = _c_problem()
    width = 3 * len(shared)
    out = {}
    for path in ("fused", "resident"):
        sol, _, _ = _solver(None, c["mesh"], **kw)
        sol.set_resident_kernel(path == "resident")
        sol.peer_attach_loopback(3)
        sol.set_state(c["d0"], c["dn"], se.TN0)
        hist = torch.full((2510, width), -7.0, dtype=torch.float64, device="cuda")
        sol.step_peer(2500, hist, 3)
        sol.synchronize()
        g0, gn, _ = sol.get_state()
        h = hist.cpu().numpy()
        assert (h[:3] == -7.0).all() and (h[2503:] == -7.0).all() and not (h[3:2503] == -7.0).any(), path
        assert np.array_equal(h[2502], g0[_dofs(shared), 0]), path  # last history row = shared dofs of the final state
        out[path] = (g0, gn, h[3:2503])
        sol.close()
    for a, b in zip(out["fused"], out["resident"]):
        e = rel_l2(b, a)
        print(f"\npeer loop-back, 2500 steps: resident against fused {e:.2e} (bar 1e-12)")
        assert e < 1e-12


# ---- D. the two counter wraps (diagnostic build, child process) -------------------------------------------------------------------
def _run_child(which, tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from _diag import diag_library_path

    code = ("import sys\n"
            f"sys.path[:0] = [{os.path.join(REPO, 'tests')!r}, {REPO!r}]\n"
            "import step_edges\n"
            f"step_edges.child_{which}()\n")
    env = dict(os.environ, SAA_LIB_PATH=diag_library_path())
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    print("\n" + r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]


def test_resident_stamps_start_over_before_they_wrap(tmp_path):
    """ps_steps preset 300 below 0x7fff0000 (diagnostic build only): calls of 400 and 2000 steps - the stamped entries are
    reset between two launches and the count starts over; state against the fused kernel at 1e-12."""
    _run_child("stamp_wrap", tmp_path)


def test_peer_sequence_wraps_with_alternating_parities(tmp_path):
    """peer_seq preset 300 below 2^32 (diagnostic build only), loop-back attach, step_peer in calls that end before,
    straddle and follow the wrap: the resident path hands over to one launch per step and takes over again, the sequence
    skips 0 AND keeps its parity alternating (after 0xffffffff comes 2); history and state against a run far from the
    wrap at 1e-12."""
    _run_child("peer_seq_wrap", tmp_path)
