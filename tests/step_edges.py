"""Shapes that put the step kernels (csrc/saa_kernels.hip: fused_step_kernel, persistent_steps_kernel = the resident
kernel, det_items_kernel / det_nodes_kernel) on both sides of their per-thread sweep depths, of the resident kernel's LDS
limit and of whole 64-lane waves - and, per regime, the predicate over the plan's statistics that PROVES a shape is where
it claims to be.  Shared by test_step_edge_shapes.py (no GPU: asserts the predicates) and test_gpu_step_edges.py (runs the
kernels there against the oracle).

The plan does not depend on ``threads``, so everything here is evaluated on the host (``plan_host_stats``: maxima of the
owned / local node counts over the blocks, totals of halo nodes and work items, i.e. means per block;
``plan_host_block_maxima``: the largest halo, item, interior and boundary lists and the smallest owned count and halo).

Sweep depths, restated from the kernels (a list of L entries is swept by T threads in ceil(L / T) sweeps):
  fused kernel      first 2 sweeps of the owned dofs (kPreOwn), of the halo dofs (kPreHalo) and of the interior items
                    (kPreConn) travel in registers, the rest take a separately written loop each;
  resident kernel   staging keeps 3 sweeps of owned dofs (kOwnSweeps) and 2 of halo dofs (kHaloSweeps) in registers; per
                    step 2 sweeps of stamped halo entries are prefetched (kPH), the others are only ever read on the
                    retry path; the first interior round and 2 sweeps of the second item phase sit in registers."""
import functools
from dataclasses import dataclass
import numpy as np

LDS_LIMIT = 160 * 1024   # persistent_lds_bytes: above it the resident kernel is refused
RESIDENT_CHUNK = 1000    # kPersistChunk: steps per resident launch


def make_mesh(mesh_id):
    """``beamN`` = structured_beam(N), ``delaunayN`` = delaunay_beam(N)."""
    from synchronization_avoiding_algorithms_amd.mesh import delaunay_beam, structured_beam

    if mesh_id.startswith("delaunay"):
        return delaunay_beam(int(mesh_id[len("delaunay"):]))
    return structured_beam(int(mesh_id[len("beam"):]))


def resident_lds_bytes(st, mx):
    """persistent_lds_bytes of csrc/saa_kernels.hip restated: the block image of the fused kernel (6 doubles per local
    node, 3 per owned node) plus d^(n-1), nodal mass and load, the tags, the work items and the halo's entry indices.
    Returns the bytes BEFORE the limit check (the library returns 0 above the limit)."""
    ml, mo = st["max_local"], st["max_owned"]
    raw = 8 * ((6 * ml + 3 * mo) + 3 * mo + 2 * mo) + 8 * max(mx["max_items"], 1) + 4 * mo + 12 * max(mx["max_halo"], 1) + 16
    return raw, (raw + 15) // 16 * 16


# ---- regimes: name -> predicate(st, mx, threads) -----------------------------------------------------------------------
# st = plan_host_stats, mx = plan_host_block_maxima, t = threads of a workgroup (the automatic choice when the shape says 0)
def _mean_halo3(st):
    return 3 * st["n_halo_total"] / st["n_blocks"]


def _mean_items(st):
    return st["n_items"] / st["n_blocks"]


REGIMES: dict = {
    # some block has more owned dofs than the resident kernel's three register sweeps (hence the fused kernel's two)
    "deep_own": lambda st, mx, t: 3 * st["max_owned"] > 3 * t,
    # the mean halo already exceeds two sweeps, so some block's does: both kernels' halo tails, and in the resident kernel
    # halo dofs that are read through the retry path only
    "deep_halo": lambda st, mx, t: _mean_halo3(st) > 2 * t and 3 * mx["max_halo"] > 2 * t,
    # some block has more than 3 t items: whatever its interior share, its second phase (all items but the <= t of the
    # first round) has more than 2 t slots - the resident kernel's item tail
    "deep_items": lambda st, mx, t: _mean_items(st) > 3 * t and mx["max_items"] > 3 * t,
    # the fused kernel's interior tail (more interior items than its two register-held sweeps), and with it a resident
    # kernel whose second phase starts with left-over interior items (n_ir > 0, padded to whole waves)
    "deep_interior": lambda st, mx, t: mx["max_interior"] > 2 * t,
    # every list of every block is shorter than the workgroup: idle lanes holding the null item, n_pre < threads, n_ir = 0,
    # clamped prefetch indices; some block has fewer interior items than one wave, where the wave-balance shift of the
    # fused kernel is taken modulo the number of waves
    "all_shallow": lambda st, mx, t: (3 * st["max_local"] <= t and _mean_items(st) < t and mx["max_items"] <= t
                                       and mx["max_interior"] < 64 and st["n_blocks"] > 1 and mx["min_halo"] > 0),
    "no_halo": lambda st, mx, t: st["n_blocks"] == 1 and st["n_halo_total"] == 0 and mx["max_halo"] == 0,
    # a workgroup of whole waves whose count is not a power of two, on a plan whose blocks do exchange halo values
    # (37 workgroups, at most one per CU: whether they are co-resident is for the census to say, not for the integer
    # division by threads / 256 in persistent_max_blocks, which only matters with several workgroups per CU)
    "threads_not_pow2": lambda st, mx, t: (t % 64 == 0 and 64 < t <= 1024 and (t & (t - 1)) != 0
                                            and st["n_blocks"] > 1 and mx["min_halo"] > 0),
    # the resident image nearly fills the LDS / is just too large for it (while the fused kernel's image still fits, so
    # that the plan builder does not halve the blocks)
    "lds_just_under": lambda st, mx, t: LDS_LIMIT - 8 * 1024 <= resident_lds_bytes(st, mx)[0] <= LDS_LIMIT,
    "lds_just_over": lambda st, mx, t: (LDS_LIMIT < resident_lds_bytes(st, mx)[0] <= LDS_LIMIT + 8 * 1024
                                         and st["lds_bytes"] <= LDS_LIMIT),
}


@dataclass(frozen=True)
class Shape:
    name: str
    mesh_id: str            # see make_mesh
    block_nodes: int
    threads: int            # 0: the library chooses
    regimes: tuple          # names of REGIMES this shape is claimed (and asserted) to reach
    resident: object        # True: must run resident; False: must be refused; None: the census decides
    delaunay: bool = False  # unstructured mesh: the wider bars of test_gpu_parity.py apply
    n_blocks: int = 0       # the plan's block count (asserted: the plan builder must not silently move a shape)


SHAPES = (
    Shape("deep_all_lists-beam6-bn400-t64", "beam6", 400, 64,
          ("deep_own", "deep_halo", "deep_items", "deep_interior"), True, n_blocks=19),
    Shape("deep_all_lists-delaunay5-bn400-t64", "delaunay5", 400, 64,
          ("deep_own", "deep_halo", "deep_items", "deep_interior"), True, delaunay=True, n_blocks=12),
    Shape("all_shallow-beam5-bn24-t1024", "beam5", 24, 1024, ("all_shallow",), True, n_blocks=189),
    Shape("no_halo-beam2-one_block-t256", "beam2", 2000, 256, ("no_halo",), True, n_blocks=1),
    Shape("no_halo-beam2-one_block-t64", "beam2", 2000, 64, ("no_halo", "deep_own", "deep_items"), True, n_blocks=1),
    Shape("no_halo-beam1-automatic", "beam1", 0, 0, ("no_halo",), True, n_blocks=1),
    Shape("threads_not_pow2-beam6-bn200-t192", "beam6", 200, 192, ("threads_not_pow2",), None, n_blocks=37),
    Shape("threads_not_pow2-beam6-bn200-t320", "beam6", 200, 320, ("threads_not_pow2",), None, n_blocks=37),
    Shape("threads_not_pow2-beam6-bn200-t704", "beam6", 200, 704, ("threads_not_pow2",), None, n_blocks=37),
    Shape("threads_not_pow2-beam6-bn200-t960", "beam6", 200, 960, ("threads_not_pow2",), None, n_blocks=37),
    Shape("lds_just_under-beam8-bn1100", "beam8", 1100, 0, ("lds_just_under",), True, n_blocks=15),
    Shape("lds_just_over-beam8-bn1200", "beam8", 1200, 0, ("lds_just_over",), False, n_blocks=14),
)

# the two shapes that are run once more with declared shared nodes (predicted phase, loop-back peer exchange)
SHARED_NODE_SHAPES = ("deep_all_lists-beam6-bn400-t64", "all_shallow-beam5-bn24-t1024")


def spread_nodes(n_nodes, count=12):
    """``count`` declared-shared nodes spread over the numbering (away from the clamped end): they fall into different
    blocks, some owned by interior items only, some next to a halo."""
    return np.unique(np.linspace(n_nodes / 7, 6 * n_nodes / 7, count).astype(np.int32))


def by_name(name):
    return next(s for s in SHAPES if s.name == name)


def solver_numbering(mesh):
    """(points, cells) as test_gpu_parity._serial_solver hands them to the library: the serial problem in the reference's
    first-touch numbering.  The block plan depends on the numbering, so the predicates are evaluated on THIS input."""
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes

    layouts, _ = fs.build_layouts(mesh.tets, np.zeros(len(mesh.tets), dtype=int), 1, len(mesh.points), clamp_nodes(mesh))
    return mesh.points[layouts[0].nodes], layouts[0].cells_local


def plan_facts(shape):
    """(mesh, plan_host_stats, plan_host_block_maxima, effective threads) of a shape - no GPU."""
    from synchronization_avoiding_algorithms_amd.solver import plan_host_block_maxima, plan_host_stats

    mesh = make_mesh(shape.mesh_id)
    pts, cells = solver_numbering(mesh)
    st = plan_host_stats(pts, cells, shape.block_nodes)
    mx = plan_host_block_maxima(pts, cells, shape.block_nodes)
    return mesh, st, mx, shape.threads or st["threads"]


# ---- the start state and its sensitivity -------------------------------------------------------------------------------
def rough_state(n_dof, dirichlet, seed):
    """Every dof moving from step 1 on (as in test_synthetic_beam_against_oracle): amplitudes 1e-4 / 1e-6."""
    rng = np.random.default_rng(seed)
    d0 = rng.uniform(-1e-4, 1e-4, size=(n_dof, 1))
    dn = d0 + rng.uniform(-1e-6, 1e-6, size=(n_dof, 1))
    d0[dirichlet] = 0
    dn[dirichlet] = 0
    return d0, dn


def oracle_steps(fo, rp, dt, d0, dn, tn, n_steps, K=None, stale=None):
    """``n_steps`` of the oracle's explicit step.  ``stale = (step, dof)``: in the force evaluation of that one step the
    field is read with ``dof`` one step old - the smallest data-flow error a step kernel can make."""
    K = rp.K if K is None else K
    o0, on = d0, dn
    for s in range(n_steps):
        if stale is not None and s == stale[0]:
            seen = o0.copy()
            seen[stale[1]] = on[stale[1]]
            o1 = fo.cd_update(K.dot(seen), rp.F, rp.l_M, o0, on, dt, tn, 0.5, rp.dirichlet)  # only the FORCE sees it
        else:
            o1 = fo.explicit_step(K, rp.F, rp.dirichlet, tn, dt, o0, on, rp.l_M, 0.5)
        on, o0 = o0, o1
        tn = tn + dt
    return o0, on, tn


def stale_read_sensitivity(fo, rp, dt, d0, dn, tn, n_steps, clean_d0, seed, K=None):
    """Smallest relative change of the final d0 over the two single stale reads the issue names (one free dof, at the
    middle step and at the last step but one)."""
    from conftest import rel_l2

    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(len(d0)), rp.dirichlet)
    worst = np.inf
    for step in (n_steps // 2, n_steps - 2):
        dof = int(rng.choice(free))
        got, _, _ = oracle_steps(fo, rp, dt, d0, dn, tn, n_steps, K=K, stale=(step, dof))
        worst = min(worst, rel_l2(got, clean_d0))
    return worst


def oracle_steps_loopback(fo, rp, dt, d0, dn, tn, n_steps, sh_dof, world):
    """The operator saa_peer_attach_loopback documents: every shared node is updated with ``world`` x its local force,
    summed in rank order ((f + f) + f for three holders); returns the state and the history of the shared dofs."""
    o0, on = d0, dn
    hist = np.zeros((n_steps, len(sh_dof)))
    for s in range(n_steps):
        f = rp.K.dot(o0)
        own = f[sh_dof].copy()
        for _ in range(world - 1):
            f[sh_dof] = f[sh_dof] + own
        o1 = fo.cd_update(f, rp.F, rp.l_M, o0, on, dt, tn, 0.5, rp.dirichlet)
        hist[s] = o1[sh_dof, 0]
        on, o0 = o0, o1
        tn = tn + dt
    return o0, on, tn, hist


N_STEPS, TN0 = 200, 0.25


@functools.lru_cache(maxsize=None)
def oracle_case(mesh_id):
    """One mesh of the table with the oracle's serial problem, the rough start state and the oracle's state after N_STEPS
    steps from it (shapes on the same mesh share it)."""
    from oracle import fem_oracle as fo

    mesh = make_mesh(mesh_id)
    ranks, dt, _, _ = fo.setup_problem(mesh.points, mesh.tets, mesh.triangles, 1, np.zeros(len(mesh.tets), dtype=int))
    rp = ranks[0]
    d0, dn = rough_state(3 * len(rp.nodes), rp.dirichlet, seed=len(rp.nodes))
    o0, on, tn = oracle_steps(fo, rp, dt, d0, dn, TN0, N_STEPS)
    return {"mesh": mesh, "rp": rp, "dt": dt, "d0": d0, "dn": dn, "o0": o0, "on": on, "tn": tn}


def bars(shape):
    """(operator, trajectory) bars of test_gpu_parity.py: 1e-13 / 1e-11, on Delaunay meshes 1e-12 / 1e-10."""
    return (1e-12, 1e-10) if shape.delaunay else (1e-13, 1e-11)


# ---- the two counter wraps: bodies of the child processes of test_gpu_step_edges.py (diagnostic build of the library) ----
def _debug_counters(sol):
    """(peer_seq, ps_steps, parity_repeats, resident_launches) of a handle: saa_debug_counters, diagnostic build only."""
    import ctypes as C

    from synchronization_avoiding_algorithms_amd import _lib

    fn = _lib.load().saa_debug_counters
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    seq, steps, rep, launches = C.c_uint32(), C.c_uint32(), C.c_int64(), C.c_int64()
    _lib.check(fn(sol._h, C.byref(seq), C.byref(steps), C.byref(rep), C.byref(launches)))
    return seq.value, steps.value, rep.value, launches.value


def _wrap_problem():
    import os

    from test_gpu_parity import _serial_solver

    c = oracle_case("beam5")
    shared = spread_nodes(len(c["rp"].nodes))
    kw = dict(shared_local=shared, shared_slots=np.arange(len(shared), dtype=np.int32), n_global_shared=len(shared))

    def make(**env):
        for k in ("SAA_PRESET_PS_STEPS", "SAA_PRESET_PEER_SEQ"):
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})  # read once, when the handle is created
        sol = _serial_solver(c["mesh"], **kw)[0]
        sol.set_option("wait_timeout_s", 5.0)
        sol.set_state(c["d0"], c["dn"], TN0)
        return sol

    return c, shared, make


def child_stamp_wrap():
    from conftest import rel_l2

    c, _, make = _wrap_problem()
    preset = 0x7fff0000 - 300
    fused = make()
    fused.set_resident_kernel(False)
    sol = make(SAA_PRESET_PS_STEPS=preset)
    assert sol.resident_kernel_info()["capable"]
    assert _debug_counters(sol)[1] == preset
    for k, want_steps, want_launches in ((400, preset + 400, 1), (2000, 2000, 3)):
        fused.step(k)
        sol.step(k)
        sol.synchronize()
        _, steps, _, launches = _debug_counters(sol)
        # first call: one launch, the count passes 0x7fff0000; second call: the entries are reset BEFORE its first launch
        # and the count starts over, so that it ends at the call's own 2000 steps
        assert (steps, launches) == (want_steps, want_launches), (k, steps, launches)
        (a0, an, ta), (b0, bn, tb) = fused.get_state(), sol.get_state()
        e0, en = rel_l2(b0, a0), rel_l2(bn, an)
        print(f"stamp wrap: after the call of {k} steps the count is {steps:#x}; resident against fused d0 {e0:.2e} dn {en:.2e}")
        assert ta == tb and e0 < 1e-12 and en < 1e-12
    assert preset + 400 > 0x7fff0000
    fused.close()
    sol.close()


def child_peer_seq_wrap():
    import torch

    from conftest import rel_l2

    c, shared, make = _wrap_problem()
    width = 3 * len(shared)
    preset = 2 ** 32 - 300
    calls = (100, 150, 100, 100)  # ends 200 below the wrap; 50 below; straddles it (one launch per step); follows it
    runs = {}
    for name, env in (("far", {}), ("near", {"SAA_PRESET_PEER_SEQ": preset})):
        sol = make(**env)
        assert sol.resident_kernel_info()["capable"]
        sol.peer_attach_loopback(3)
        seq0 = _debug_counters(sol)[0]
        assert seq0 == (preset if name == "near" else 0)
        hist = torch.zeros((sum(calls), width), dtype=torch.float64, device="cuda")
        row, seen = 0, []
        for k in calls:
            sol.step_peer(k, hist, row)
            sol.synchronize()
            row += k
            seq, _, repeats, launches = _debug_counters(sol)
            seen.append((seq, launches))
            assert repeats == 0, (name, k, repeats)  # no two consecutive exchanges in the same half of the inboxes
        if name == "far":
            assert seen == [(100, 1), (250, 2), (350, 3), (450, 4)], seen
        else:
            # 2^32 - 200 and 2^32 - 50 through the resident kernel; then 49 exchanges up to 0xffffffff, the next one is
            # number 2 (not 0 = "never written", not 1 = the parity of 0xffffffff again) and 50 more: 52, all of them one
            # launch per step; then resident again
            assert seen == [(2 ** 32 - 200, 1), (2 ** 32 - 50, 2), (52, 2), (152, 3)], seen
        g0, gn, tn = sol.get_state()
        runs[name] = (g0, gn, hist.cpu().numpy(), tn)
        sol.close()
    assert runs["far"][3] == runs["near"][3]
    for what, a, b in zip(("d0", "dn", "history"), runs["far"], runs["near"]):
        e = rel_l2(b, a)
        print(f"peer sequence wrap: {what} against the run far from the wrap {e:.2e} (bar 1e-12)")
        assert e < 1e-12
