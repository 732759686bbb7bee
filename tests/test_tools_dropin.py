"""The drop-in ``Tools`` package: same names / signatures / orderings as the reference's (CPU parts)."""
import numpy as np

from conftest import load_golden, rel_l2
from oracle import fem_oracle as fo
from synchronization_avoiding_algorithms_amd.Tools import Distributed_tools as DT
from synchronization_avoiding_algorithms_amd.Tools import Mat_construction as MC
from synchronization_avoiding_algorithms_amd.Tools import commons as CM


def test_commons(beam_coarse):
    assert CM.linear_ramp(0.3) == 0.3 and CM.linear_ramp(1.7) == 1.0
    lmd, mu = fo.lame(1e6, 0.3)
    el = CM.elasticity(lmd, mu, 1, 0.5, True)
    assert np.array_equal(el.D(), fo.elasticity_D(lmd, mu))
    assert np.array_equal(el.f(None, 0.25).ravel(), [0.0, -0.125, -0.125])
    assert CM.node_to_dof(3, [0, 1, 2], [2, 0]) == [6, 7, 8, 0, 1, 2]
    assert CM.node_to_dof(3, [1], [4]) == [13]
    dt = 0.9 * CM.Meshsize(beam_coarse.tets, beam_coarse.points) / np.sqrt(1e6 / 1 / (1 - 0.3 ** 2))
    assert dt == 0.00024784067462642383  # Results/plotter.py:25
    T = CM.Time_integration_displacement(0.5, 0.1, 1, 2)
    assert T.tn_plus_1() == 0.6


def test_partition_helpers_match_reference_orderings(beam_coarse):
    g = load_golden("tworank_trajectory.npz")
    lists = []
    for r in range(2):
        ele, nodes = DT.rankwise_dist(r, g["epart"], beam_coarse.points, beam_coarse.tets)
        assert ele == g[f"r{r}_local_elements"].tolist() and nodes == g[f"r{r}_local_nodes"].tolist()
        lists.append(nodes)
    shared = [DT.find_shared_nodes(r, 2, [len(v) for v in lists], lists) for r in range(2)]
    for r in range(2):
        assert shared[r] == g[f"r{r}_shared_nodes"].tolist()
        dn = load_golden("serial_setup.npz")["dirichlet_nodes"]
        assert DT.Dirichlet_rank_dist(dn, lists[r]) == g[f"r{r}_local_dirichlet"].tolist()
        assert DT.local_mat_node(shared[r], lists[r]) == fo.local_index(shared[r], lists[r]).tolist()
    assert np.array_equal(DT.sort_shared(shared), g["Global_shared"])


def test_lumped_mass_and_preassembled_load(beam_coarse):
    g = load_golden("serial_setup.npz")
    lmd, mu = fo.lame(1e6, 0.3)
    M, K, F = MC.Global_Assembly_no_bc(1, beam_coarse.tets, beam_coarse.points,
                                       CM.elasticity(lmd, mu, 1, 0.5, False), 0)
    assert K is None
    assert rel_l2(CM.lumping_to_vec(M), g["lumped_M"]) < 1e-14
    assert rel_l2(F, g["F_pre"]) < 1e-14
    # consistent mass entries against the reference's Local_MKF on a few elements
    e = load_golden("element_ops.npz")
    Md = M.toarray()
    el = int(e["elements"][0])
    dof = fo.node_to_dof(beam_coarse.tets[el])
    # the assembled block contains this element's contribution: check symmetry + positive row sums instead
    assert np.allclose(Md, Md.T) and (Md.sum(axis=1) > 0).all()
    assert np.isclose(Md.sum() / 3, 25.0)


def test_global_assembly_matches_the_reference(beam_coarse):
    """``Global_Assembly`` (Mat_construction.py:155-196) as the drivers call it: Data_prepare.py:183 (ramped load at
    t = 0 and later on the ramp) and Steady_solvers.py:14 (un-ramped, steady=True); dense for the reference's mesh so
    that the drivers' ``np.linalg.solve(M, F - K@d0)`` keeps working, CSR on request."""
    from scipy.sparse import csr_matrix, issparse

    g = load_golden("global_assembly.npz")
    lmd, mu = fo.lame(1e6, 0.3)
    dirichlet = g["dirichlet_dofs"].tolist()
    for name, (ramped, t, steady) in {"dyn": (True, 0, False), "dyn_t04": (True, 0.4, False),
                                      "steady": (False, None, True)}.items():
        M, K, F = MC.Global_Assembly(1, beam_coarse.tets, beam_coarse.points, dirichlet,
                                     CM.elasticity(lmd, mu, 1, 0.5, ramped), t, steady=steady)
        assert isinstance(M, np.ndarray) and isinstance(K, np.ndarray) and F.shape == (330, 1)
        for tag, A in (("M", M), ("K", K)):
            ref = csr_matrix((g[f"{name}_{tag}_data"], g[f"{name}_{tag}_indices"], g[f"{name}_{tag}_indptr"]),
                             shape=A.shape).toarray()
            assert np.abs(A - ref).max() <= 2e-15 * np.abs(ref).max()
            assert not A[dirichlet].any() and not A[:, dirichlet].any()
        assert np.abs(F - g[f"{name}_F"]).max() <= 1e-15
    Ms, Ks, Fs = MC.Global_Assembly(1, beam_coarse.tets, beam_coarse.points, dirichlet,
                                    CM.elasticity(lmd, mu, 1, 0.5, False), None, steady=True, sparse=True)
    assert issparse(Ms) and issparse(Ks) and np.array_equal(Ks.toarray(), K) and np.array_equal(Fs, F)
    # the ghost-step solve of Data_prepare.py:183-191 written against the drop-in: zero load at t = 0 -> a0 = 0
    M, K, F = MC.Global_Assembly(1, beam_coarse.tets, beam_coarse.points, dirichlet, CM.elasticity(lmd, mu, 1, 0.5, True), t=0)
    for dof in dirichlet:
        M[dof, dof] = 1
        F[dof] = 0
    a0 = np.linalg.solve(M, F - K @ np.zeros((330, 1)))
    assert not a0.any()


def test_shape_functions_and_quadrature_match_the_reference():
    from synchronization_avoiding_algorithms_amd.Tools import Qudrature as Q
    from synchronization_avoiding_algorithms_amd.Tools import Shape_function_Deriv as S

    g = load_golden("shape_quadrature.npz")
    for n in (2, 3):
        nodes, weights = Q.Gauss_Legendre(n)
        assert np.array_equal(nodes, g[f"q{n}_nodes"]) and np.array_equal(weights, g[f"q{n}_weights"])
    assert abs(Q.Gauss_Legendre(2)[1].sum() - 1.0 / 6) < 1e-17
    assert np.array_equal(np.array([S.Shape_Function(1, x) for x in g["xi"]]), g["N"])
    assert np.array_equal(np.array([S.Shape_Deri(1, x) for x in g["xi"]]), g["dN"])
    for e, P in enumerate(g["P"]):
        for q, x in enumerate(g["xi"]):
            assert np.abs(S.Jacobian(1, P, x) - g["J"][e, q]).max() < 1e-15
            assert S.IsoparametricMap(1, P, x).shape == (3, 1)
            assert np.abs(S.IsoparametricMap(1, P, x) - g["X"][e, q]).max() < 4e-15
    # p = 2 (10-node tets with curved edges) and the 14-point rule: not on the dynamic path, part of the Tools surface
    g2 = load_golden("shape_quadrature_p2.npz")
    nodes, weights = Q.Gauss_Legendre(4)
    assert np.array_equal(nodes, g2["q4_nodes"]) and np.array_equal(weights, g2["q4_weights"])
    assert abs(weights.sum() - 1.0 / 6) < 1e-15
    assert np.abs(np.array([S.Shape_Function(2, x) for x in g2["xi"]]) - g2["N"]).max() < 1e-15
    assert np.abs(np.array([S.Shape_Deri(2, x) for x in g2["xi"]]) - g2["dN"]).max() < 1e-15
    assert np.abs(np.array([S.Shape_Function(2, x) for x in g2["xi"]]).sum(axis=1) - 1.0).max() < 1e-15  # partition of unity
    for e, P in enumerate(g2["P"]):
        for q, x in enumerate(g2["xi"]):
            assert np.abs(S.Jacobian(2, P, x) - g2["J"][e, q]).max() < 1e-14
            assert np.abs(S.IsoparametricMap(2, P, x) - g2["X"][e, q]).max() < 1e-14
    import pytest

    with pytest.raises(NotImplementedError):
        S.Shape_Function(3, [0.1, 0.1, 0.1])
    with pytest.raises(NotImplementedError):
        Q.Gauss_Legendre(5)


def test_every_tools_name_the_reference_drivers_use_exists():
    """the reference's four driver scripts run against this package's ``Tools``.  The names
    they use and the ``Tools`` modules that define them were read from the reference's sources as text
    (golden/tools_names.json, written by golden/make_golden_names.py)."""
    import importlib
    import json
    import os

    from conftest import GOLDEN

    with open(os.path.join(GOLDEN, "tools_names.json")) as fh:
        rec = json.load(fh)
    assert rec["drivers"] == ["Data_prepare.py", "Online_predictor.py", "Shared_extraction.py", "Model_training.py"]
    used = rec["used"]
    assert len(used) >= 20
    for name in sorted(used):
        mods = [importlib.import_module(f"synchronization_avoiding_algorithms_amd.Tools.{m}") for m in used[name]]
        assert any(hasattr(m, name) for m in mods), name
