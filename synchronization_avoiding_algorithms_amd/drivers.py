"""The reference's driver scripts as functions + CLIs (one process per GPU).

``Data_prepare.py`` -> :func:`data_prepare`, ``Shared_extraction.py`` -> :func:`shared_extraction`,
``Online_predictor.py`` -> :func:`online_predictor`, plus :func:`modal` (stable time step and lowest modes, the
reference's ``Eigen_mode``), :func:`dynamics` (the explicit run of one whole mesh on one GPU for either element order;
the reference has none for ``p = 2``), :func:`stress` (stress recovery from the saved trajectories) and :func:`estimate` (the
Zienkiewicz-Zhu estimate of the stress error of the mesh, the scale for the error of the modelled run; neither has a
counterpart in the reference; :func:`stress_finite` and :func:`estimate_finite` are the two at finite strain, on the run of
:func:`dynamics` with a nonlinear material, :func:`stress_p2` and :func:`estimate_p2` the two for quadratic tetrahedra; these
four are thin calls into one whole-mesh stress driver and one whole-mesh estimate driver, :func:`_whole_stress` and
:func:`_whole_estimate`, which take the order and the material); same artefact names under ``Results/`` and
``Distributed_save/``, same constants by default.  Launch like the reference's
``mpirun -np P python3 X.py``:

    python -m torch.distributed.run --nproc-per-node P --master-addr 127.0.0.1 \\
        -m synchronization_avoiding_algorithms_amd.drivers data_prepare --mesh Mesh_info/beam_coarse.vtk

Differences, all forced by the environment or by scale: the element partition comes from
``mesh.slab_partition`` / ``rcb_partition`` (ParMETIS is not available); the steady solve of
``Data_prepare.py:158-168`` (a dense O(N^3) diagnostic that never feeds the time loop) is not run; the
ghost step is the exact zero the reference obtains for a ramped load (``Data_prepare.py:178-191``).
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import predictor as pr
from . import results_io as rio
from .distributed import PartitionedSolver, run_hybrid
from .mesh import rcb_partition, read_vtk, slab_partition, structured_beam

# constants of Data_prepare.py:35-50 / Online_predictor.py:38-63
DEFAULTS = dict(E=1e6, nu=0.3, rho=1.0, fz=0.5, alpha=0.5, gamma=0.9)
STEADY_PATH = "Results/Static/steady_distributed.vtk"   # Data_prepare.py:25,168
PATHS = dict(local_nodes="Results/Rankwised_Data/Rank={r}_local_nodes.csv",
             shared="Results/Shared_Data/Rank={r}_shared.csv",
             global_shared="Results/Shared_Data/Global_shared.csv",
             elements="Results/Rankwised_Element/Rank={r}_elements.csv",
             truth="Results/Dynamics/Local-rank-{r}.hdf5",
             dynamics="Results/Dynamics/Displacement_order{p}.hdf5",
             energy="Results/Dynamics/Energy_order{p}.hdf5",
             time="Results/Dynamics/Time_order{p}.npz",
             modeled="Results/Dynamics/Modeled_Local-rank-{r}.hdf5",
             shared_traj="Results/sol_on_shared/rank={r}-shared_dof.hdf5",
             model="Distributed_save/Rank-{r}/nB-{nB}-nH-{nH}-Lr-{lr}-filter={ns}/model.pth",
             stress_vtk="Results/Stress/Stress-col-{j}.vtk",
             modeled_stress_vtk="Results/Stress/Modeled_Stress-col-{j}.vtk",
             stress_history="Results/Stress/history.npz",
             estimate_vtk="Results/Stress/Estimate-col-{j}.vtk",
             stress_vtk_p2="Results/Stress/Stress-order2-col-{j}.vtk",
             stress_history_p2="Results/Stress/history-order2.npz",
             estimate_vtk_p2="Results/Stress/Estimate-order2-col-{j}.vtk",
             stress_vtk_fs="Results/Stress/Stress-{material}-order{p}-col-{j}.vtk",
             stress_history_fs="Results/Stress/history-{material}-order{p}.npz",
             estimate_vtk_fs="Results/Stress/Estimate-{material}-order{p}-col-{j}.vtk")


def _dist_env():
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        import torch

        backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist.init_process_group(backend)
    return rank, world, local


def make_partition(mesh, world, how="slab"):
    if world == 1:
        return np.zeros(len(mesh.tets), dtype=np.int64)
    if how == "graph":
        from .mesh import graph_partition

        return graph_partition(mesh, world)
    return slab_partition(mesh, world) if how == "slab" else rcb_partition(mesh, world)


# Largest trajectory matrix kept on the GPU by the drivers (bytes); beyond it the host collects column by column.
DEVICE_TRAJECTORY_BUDGET = 32 << 30


def _device_recorder(part, n_steps, save_every):
    """``d1_save`` (``Data_prepare.py:219,236-240``) as a device matrix filled by the step kernels themselves
    (``saa_set_recorder``), or None when the solver has no recorder / the matrix would not fit the budget."""
    import torch

    n_cols = int(n_steps / save_every)
    n_dof = 3 * len(part.layout.nodes)
    if (part.tensor_device.type != "cuda" or not hasattr(part.solver, "set_recorder") or n_cols <= 0
            or 8 * n_dof * n_cols > DEVICE_TRAJECTORY_BUDGET):
        return None
    traj = torch.zeros((n_dof, n_cols), dtype=torch.float64, device=part.tensor_device)
    part.solver.set_recorder(traj, save_every, 0)
    return traj


def _saver(part, n_steps, save_every):
    store = np.zeros((3 * len(part.layout.nodes), int(n_steps / save_every)))
    state = {"counter": 0}

    def save(i, p):
        if i % save_every == 0 and state["counter"] < store.shape[1]:
            store[:, state["counter"]] = p.get_state()[0][:, 0]
            state["counter"] += 1

    return store, save


def data_prepare(mesh, n_steps=100000, save_every=1, out_dir=".", rank=0, world=1, partition="slab",
                 device=0, verbose=False, epart=None, **part_kw):
    """``Data_prepare.py:82-246``: partition, artefact CSVs, synchronised explicit run, trajectory file."""
    epart = make_partition(mesh, world, partition) if epart is None else epart
    part = PartitionedSolver(mesh.points, mesh.tets, mesh.triangles, epart, rank, world, device=device,
                             **{**DEFAULTS, **part_kw})
    lay = part.layout
    rio.save_int_list(os.path.join(out_dir, PATHS["shared"].format(r=rank)), lay.shared_nodes)
    rio.save_int_list(os.path.join(out_dir, PATHS["local_nodes"].format(r=rank)), lay.nodes)
    rio.save_int_list(os.path.join(out_dir, PATHS["elements"].format(r=rank)), lay.elements)
    if rank == 0:
        rio.save_int_list(os.path.join(out_dir, PATHS["global_shared"]), part.global_shared)
        if verbose:
            print("Time-step size is: " + str(part.dt))
    traj = _device_recorder(part, n_steps, save_every)
    if traj is not None:  # the kernels fill the trajectory; the whole run is a handful of launches
        part.step_synced(n_steps)
        part.solver.synchronize()
        store = traj.cpu().numpy()
        part.solver.set_recorder(None)
    else:
        store, save = _saver(part, n_steps, save_every)
        i = 0
        while i < n_steps:  # saved steps are i % save_every == 0 (Data_prepare.py:238-240)
            n = 1 if i % save_every == 0 else min(save_every - i % save_every, n_steps - i)
            part.step_synced(n)
            i += n
            save(i - 1, part)
    path = rio.save_displacement(os.path.join(out_dir, PATHS["truth"].format(r=rank)), store)
    part.close()
    return path, store


def _quadratic(mesh):
    """The mesh with 10-node cells: as read if the file holds ``tetra10``, else elevated (``mesh.to_quadratic``)."""
    from .mesh import to_quadratic

    return mesh if "tetra10" in mesh.cells_dict else to_quadratic(mesh)


def steady_state(mesh, out_dir=".", device=0, tol=1e-12, verbose=False, E=None, nu=None, rho=None, fz=None, order=1):
    """``Data_prepare.py:157-168`` (rank 0 in the reference): the steady solution ``d = K^-1 F`` of the whole mesh
    under the un-ramped load, written as point data of ``Results/Static/steady_distributed.vtk``.  Matrix-free
    preconditioned CG on one GPU (:mod:`steady`) instead of the dense solve.  ``order=2``: quadratic tetrahedra (what the
    reference's ``p = 2`` gives), clamped on every node of ``x = 0``, written with type-24 cells."""
    from . import fem_setup as fs
    from .mesh import clamp_nodes
    from .solver import HipExplicitSolver
    from .steady import steady_solve, stiffness_diagonal, write_vtk_point_data

    E = DEFAULTS["E"] if E is None else E
    nu = DEFAULTS["nu"] if nu is None else nu
    rho = DEFAULTS["rho"] if rho is None else rho
    fz = DEFAULTS["fz"] if fz is None else fz
    lmd, mu = fs.lame(E, nu)
    if order == 2:
        from .mesh import plane_nodes
        from .modal import ModalOperator
        from .steady import steady_solve_operator

        mesh = _quadratic(mesh)
        with ModalOperator(mesh.points, mesh.tets10, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, rho, device) as op:
            d, iters, rel = steady_solve_operator(op, op.load((0.0, -fz, -fz)), tol=tol)
        d = d.reshape(-1, 1)
        if verbose:
            print(f"steady solve (order 2): {iters} CG iterations, relative residual {rel:.2e}, max|d| = {np.abs(d).max():.6e}")
        return write_vtk_point_data(os.path.join(out_dir, STEADY_PATH), mesh.points, mesh.tets10, d), d
    if order != 1:
        raise ValueError("order must be 1 or 2")
    lumped, fpre, min_edge = fs.device_setup_fields(mesh.points, mesh.tets, rho, fz, device)
    dirichlet = fs.node_to_dof(clamp_nodes(mesh))
    sol = HipExplicitSolver(mesh.points, mesh.tets, lumped, fpre, dirichlet, lmd, mu,
                            fs.dt_from_min_edge(min_edge, E, nu, rho, DEFAULTS["gamma"]), DEFAULTS["alpha"],
                            device=device)
    d, iters, rel = steady_solve(sol, fpre, dirichlet, diag=stiffness_diagonal(mesh.points, mesh.tets, lmd, mu), tol=tol)
    sol.close()
    if verbose:
        print(f"steady solve: {iters} CG iterations, relative residual {rel:.2e}, max|d| = {np.abs(d).max():.6e}")
    path = write_vtk_point_data(os.path.join(out_dir, STEADY_PATH), mesh.points, mesh.tets, d)
    return path, d


class NotConverged(RuntimeError):
    """The Newton iteration of :func:`steady_state_nonlinear` stopped short of its tolerance; ``report`` is what it printed."""

    def __init__(self, message, report):
        super().__init__(message)
        self.report = report


def steady_state_nonlinear(mesh, out_dir=".", device=0, material="svk", order=1, fz=None, load_steps=1, tol=1e-8, E=None,
                           nu=None, rho=None):
    """The static equilibrium ``f_int(d) = F`` of a finite-strain material (``svk``, ``neo_hookean``) on the whole mesh of
    either order, clamped on every node of ``x = 0`` under the un-ramped load ``(0, -fz, -fz)`` (the clamp and load of
    ``steady_state --order 2``): Newton-PCG on the operator handle (:func:`steady.newton_solve_operator`), written to
    ``Results/Static/steady_distributed.vtk`` like the linear solution.  Returns ``(path, d (3n, 1), report)``; the report
    holds the order, the sizes, the material, the solver's ``info`` without its history, ``max_abs_d`` and the mean
    ``tip_deflection``, and under ``linear`` the same two figures of ``K d = F``; of the converged state also the largest
    point von Mises value of the Cauchy stress (``von_mises_max``) with its ``element``, the stored energy
    (``strain_energy``) and ``min_det_f`` (:mod:`stress`), and the file holds the recovered Cauchy stress ``sigma-xx .. -xy``
    and its ``von-mises`` as point data after the displacement.  Raises :class:`NotConverged` (after writing
    nothing) when the iteration does not reach ``tol``.  The default ``tol`` is 1e-8 of ``|F|`` in the TRUE residual (the
    linear driver's 1e-12 is the residual of the CG recurrence): on the 25 : 1 beam ``f_int`` itself is only good to about
    ``eps (L/h)^4`` = 1e-9 of ``|F|`` in float64, because an element's nodal displacements are mostly its rigid motion."""
    from . import fem_setup as fs
    from .mesh import plane_nodes
    from .modal import ModalOperator
    from .steady import newton_solve_operator, steady_solve_operator, write_vtk_point_data
    from .stress import VOIGT, QuadraticStressRecovery, StressRecovery, von_mises

    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    E = DEFAULTS["E"] if E is None else E
    nu = DEFAULTS["nu"] if nu is None else nu
    rho = DEFAULTS["rho"] if rho is None else rho
    fz = DEFAULTS["fz"] if fz is None else fz
    lmd, mu = fs.lame(E, nu)
    if order == 2:
        mesh = _quadratic(mesh)
    cells = np.asarray(mesh.tets10 if order == 2 else mesh.tets)
    points = np.asarray(mesh.points, dtype=np.float64)
    n_vert = int(cells[:, :4].max()) + 1 if len(cells) else 0
    tip = np.nonzero(np.abs(points[:n_vert, 0] - points[:, 0].max()) < 1e-9)[0]

    def figures(d):
        d = np.asarray(d).reshape(-1, 3)
        return {"max_abs_d": float(np.abs(d).max()), "tip_deflection": float(-d[tip, 1].mean())}

    with ModalOperator(points, cells, fs.node_to_dof(plane_nodes(points)), lmd, mu, rho, device) as op:
        load = op.load((0.0, -fz, -fz))
        d_lin, _, _ = steady_solve_operator(op, load, tol=1e-12)
        d, info = newton_solve_operator(op, load, material, tol=tol, load_steps=load_steps)
        report = {"order": op.order, "n_nodes": op.n_nodes, "n_elems": op.n_elems, "n_free_dofs": int(op.free.sum().item()),
                  "material": str(material).replace("-", "_"), "fz": float(fz),
                  **{k: v for k, v in info.items() if k != "residual_history"}, **figures(d), "linear": figures(d_lin)}
        if info["converged"]:
            import torch

            rec = (QuadraticStressRecovery if order == 2 else StressRecovery)(None, None, None, None, operator=op)
            el = rec.element(torch.as_tensor(np.asarray(d, dtype=np.float64).reshape(-1), device=op.torch_device),
                             energy=False, material=material, measure="cauchy")
            nodal = rec.nodal(el["sigma"]).cpu().numpy()
            report.update({"von_mises_max": float(el["von_mises_max"]),
                           "element": int(el["von_mises_argmax"]) // (4 if order == 2 else 1),
                           "strain_energy": float(el["energy_total"]), "min_det_f": float(el["det_f"].min())})
    if not info["converged"]:
        raise NotConverged(f"steady_state --material {material}: Newton stopped after {info['newton_iterations']} iterations at "
                           f"a relative residual of {info['residual']:.3e} (tolerance {tol:g}, {info['n_inverted']} inverted "
                           "elements); try more --load-steps", report)
    d = d.reshape(-1, 1)
    extra = {**{f"sigma-{c}": nodal[:, a] for a, c in enumerate(VOIGT)}, "von-mises": von_mises(nodal)}
    return write_vtk_point_data(os.path.join(out_dir, STEADY_PATH), points, cells, d, extra), d, report


def shared_extraction(out_dir=".", rank=0):
    """``Shared_extraction.py:22-40``: rows ``shared_dof`` of the rank's trajectory."""
    local = rio.load_int_list(os.path.join(out_dir, PATHS["local_nodes"].format(r=rank)))
    shared = rio.load_int_list(os.path.join(out_dir, PATHS["shared"].format(r=rank)))
    pos = {int(g): i for i, g in enumerate(local)}
    loc = np.array([pos[int(g)] for g in shared], dtype=np.int64)
    shared_dof = (3 * loc[:, None] + np.arange(3)[None, :]).ravel()
    data = rio.load_displacement(os.path.join(out_dir, PATHS["truth"].format(r=rank)))
    d = data[shared_dof, :]
    return rio.save_displacement(os.path.join(out_dir, PATHS["shared_traj"].format(r=rank)), d, compress=False), d


def online_predictor(mesh, n_steps=100000, save_every=1, out_dir=".", rank=0, world=1, partition="slab",
                     device=0, n_past=20, n_future=20, filter_size=150, hidden_size=50, nB=10,
                     learning_rate=5e-4, cut_off=0.5, model=None, scale=None, epart=None, resync_every=None,
                     resync_steps=None, **part_kw):
    """``Online_predictor.py:116-324``: warm-up with synchronisation, then LSTM-predicted halos.  ``resync_every`` /
    ``resync_steps``: synchronised steps again after every so many predicted windows (an extension, see
    :func:`distributed.run_hybrid`; None = the reference, which never synchronises again)."""
    import torch

    epart = make_partition(mesh, world, partition) if epart is None else epart
    part = PartitionedSolver(mesh.points, mesh.tets, mesh.triangles, epart, rank, world, device=device,
                             **{**DEFAULTS, **part_kw})
    if scale is None:  # Online_predictor.py:130-136
        traj = rio.load_displacement(os.path.join(out_dir, PATHS["shared_traj"].format(r=rank)))
        scale = pr.scaling_constants(traj, filter_size, n_past, n_future, cut_off)
    if model is None:  # Online_predictor.py:139-141
        mpath = os.path.join(out_dir, PATHS["model"].format(r=rank, nB=nB, nH=hidden_size, lr=learning_rate,
                                                            ns=filter_size))
        model = pr.call_model(part.tensor_device, filter_size, part.input_size, hidden_size, mpath)
    model = model.to(part.tensor_device)
    traj = _device_recorder(part, n_steps, save_every)
    store, save = (None, None) if traj is not None else _saver(part, n_steps, save_every)
    with torch.no_grad():
        hist = run_hybrid(part, n_steps, pr.DevicePredictor(model, n_past, n_future, filter_size, *scale),
                          n_past, n_future, filter_size, save=save, resync_every=resync_every,
                          resync_steps=resync_steps)
    if traj is not None:
        part.solver.synchronize()
        store = traj.cpu().numpy()
        part.solver.set_recorder(None)
    path = rio.save_displacement(os.path.join(out_dir, PATHS["modeled"].format(r=rank)), store)
    part.close()
    return path, store, hist


def modal(mesh, k=6, device=0, E=None, nu=None, rho=None, gamma=None, order=1, material="linear", fz=None, fx=0.0,
          load_steps=1):
    """Stable time step and lowest ``k`` natural frequencies of the whole mesh, clamped on ``x = 0`` like the other
    drivers (``Data_prepare.py:127-136``), on one GPU (:func:`modal.modal_report`).  Does not change how any other
    driver picks ``dt``.  ``order=2``: the frequencies of the quadratic discretisation (:func:`modal.modal_report_p2`),
    without the time-step figures of the explicit p = 1 solver.

    ``material`` ``svk`` / ``neo_hookean``: the frequencies about the equilibrium under the body force ``(fx, -fz, -fz)``
    (the Newton solve of ``steady_state --material`` in ``load_steps`` fractions, then ``K_T(u*) x = omega^2 M x``), next to
    the unstressed ones of the same handle (:func:`modal.prestressed_report`); with ``linear``, whose modes do not depend on
    the load, ``fz``, ``fx`` and ``load_steps`` are not looked at."""
    from .mesh import clamp_nodes
    from .modal import modal_report

    p = {name: DEFAULTS[name] if v is None else v for name, v in (("E", E), ("nu", nu), ("rho", rho), ("gamma", gamma))}
    if str(material).replace("-", "_") != "linear":
        from .mesh import plane_nodes
        from .modal import prestressed_report

        if order not in (1, 2):
            raise ValueError("order must be 1 or 2")
        fz = DEFAULTS["fz"] if fz is None else fz
        p.pop("gamma")
        if order == 2:
            mesh = _quadratic(mesh)
        return prestressed_report(mesh.points, mesh.tets10 if order == 2 else mesh.tets,
                                  plane_nodes(mesh.points) if order == 2 else clamp_nodes(mesh), material,
                                  load=(float(fx), -float(fz), -float(fz)), k=k, load_steps=load_steps, device=device, **p)
    if order == 2:
        from .mesh import plane_nodes
        from .modal import modal_report_p2

        mesh = _quadratic(mesh)
        p.pop("gamma")
        return modal_report_p2(mesh.points, mesh.tets10, plane_nodes(mesh.points), k=k, device=device, **p)
    if order != 1:
        raise ValueError("order must be 1 or 2")
    return modal_report(mesh.points, mesh.tets, clamp_nodes(mesh), k=k, device=device, **p)


def dynamics(mesh, n_steps=100000, save_every=1, out_dir=".", device=0, order=1, E=None, nu=None, rho=None, fz=None,
             alpha=None, gamma=None, parts=0, partition="slab", energy_every=0, material="linear", dt_check_every=0,
             dt_follow=None, dt_follow_every=10, scheme="explicit", dt_factor=10.0, newton_tol=1e-10):
    """The explicit run of the whole mesh on one GPU through the operator handle (:func:`dynamics.run_dynamics`), for
    linear (``order=1``) or quadratic tetrahedra (``order=2``: the mesh is elevated like ``steady_state --order 2``),
    clamped on every node of ``x = 0``: lumped mass of the handle (HRZ for order 2), the reference load ``(0, -fz, -fz)``
    with the ramp, ``alpha`` of ``Data_prepare.py:41`` and ``dt = gamma * 2/omega_max``.  Writes
    ``Results/Dynamics/Displacement_order{p}.hdf5`` and returns ``(path, report)``.  ``parts = P > 0``: the same run on
    the mesh cut into ``P`` parts (``partition``: slab, graph or rcb, on the vertex tetrahedra), every synchronised step
    split around the sum of the shared-node forces (:class:`dynamics.OperatorPartition`); same file.  ``energy_every = S >
    0``: the energy balance of every ``S``-th step (``T, U_{n+1/2}, U_n, W, D``, ``include/saa_hip.h``) goes to dataset
    ``Energy`` of ``Results/Dynamics/Energy_order{p}.hdf5``, and the report gains ``energy`` and ``energy_path``.
    ``material``: ``linear``, ``svk`` (St. Venant-Kirchhoff) or ``neo_hookean`` - the finite-strain element pass
    (``include/saa_hip.h``); with a nonlinear one the report gains ``material``, ``inverted`` and ``first_inverted_step``.  ``dt`` stays that of
    the LINEAR operator at the reference configuration: under large stretch the tangent stiffens, the stability limit moves,
    and the stepper does not follow it unless ``dt_follow`` asks for it.  The energy balance is defined for ``linear`` only (ValueError otherwise).
    ``dt_check_every = S > 0`` (a nonlinear material, no ``parts``): the limit ``2/omega_max`` of the tangent at the current
    state is measured every ``S`` steps and the report gains ``dt_check`` (:func:`dynamics.run_dynamics`); ``dt`` itself is
    not changed.  ``dt_follow = "certified"`` or ``"anchored"`` (a nonlinear material, no ``parts``, no energy balance): the step
    is checked before step 0 and after every ``dt_follow_every`` steps and changed by the rule of
    :meth:`dynamics.OperatorStepper.follow_time_step`; the report gains ``dt_follow`` and ``time_path``,
    ``Results/Dynamics/Time_order{p}.npz`` with ``t`` per saved column - the columns are no longer equidistant in time - and the
    ``(step, dt)`` list of the run.  The HDF5 container is what it was.
    ``scheme = "newmark"``: the same run with the implicit stepper (:func:`dynamics.run_dynamics_newmark`) at ``dt = dt_factor *
    2/omega_max`` of the linear operator, Newton tolerance ``newton_tol``; same file and keys, plus ``scheme``, ``dt_factor``,
    ``newton_iterations``, ``cg_iterations``, ``converged``, ``failed_step``.  Not with ``parts``, the energy balance, ``dt_follow`` or
    ``dt_check_every`` (ValueError).  ``scheme = "explicit"`` is the run it always was."""
    from .dynamics import run_dynamics, run_dynamics_newmark
    from .mesh import plane_nodes

    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    if scheme not in ("explicit", "newmark"):
        raise ValueError("scheme must be explicit or newmark")
    if scheme == "newmark" and ((parts and int(parts) > 0) or energy_every or dt_follow or dt_check_every):
        raise ValueError("scheme newmark runs the whole mesh without parts, energy balance, dt_follow or dt_check_every")
    p = {name: DEFAULTS[name] if v is None else v
         for name, v in (("E", E), ("nu", nu), ("rho", rho), ("fz", fz), ("alpha", alpha), ("gamma", gamma))}
    if order == 2:
        mesh = _quadratic(mesh)
    cells = mesh.tets10 if order == 2 else mesh.tets
    if scheme == "newmark":
        store, report = run_dynamics_newmark(mesh.points, cells, plane_nodes(mesh.points), n_steps, save_every, device=device,
                                             material=material, dt_factor=float(dt_factor), newton_tol=float(newton_tol), **p)
        return rio.save_displacement(os.path.join(out_dir, PATHS["dynamics"].format(p=order)), store), report
    epart = make_partition(mesh, int(parts), partition) if parts and int(parts) > 0 else None
    store, report, *table = run_dynamics(mesh.points, cells, plane_nodes(mesh.points), n_steps, save_every, device=device,
                                         epart=epart, energy_every=int(energy_every or 0), material=material,
                                         dt_check_every=int(dt_check_every or 0),
                                         **({"dt_follow": dt_follow, "dt_follow_every": dt_follow_every} if dt_follow else {}), **p)
    path = rio.save_displacement(os.path.join(out_dir, PATHS["dynamics"].format(p=order)), store)
    if dt_follow:
        times = table.pop()
        report["time_path"] = os.path.join(out_dir, PATHS["time"].format(p=order))
        np.savez(report["time_path"], **times)
    if table:
        report["energy_path"] = rio.save_displacement(os.path.join(out_dir, PATHS["energy"].format(p=order)), table[0],
                                                      dataset=rio.ENERGY_DATASET)
    return path, report


def _host_value(v):
    """A tensor of a recovery's result as a NumPy array; anything else (``measure``) as it is."""
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def _device_recovery(device=0, order=1):
    """The GPU side of the stress and estimate drivers, and its only one: a factory ``make(points, cells, lmd, mu)`` of
    objects with NumPy-in / NumPy-out ``element(X (m, n_dof))`` (the dict of :meth:`stress.StressRecovery.element`),
    ``nodal(E (m, n_elems, k))``, ``error(sigma_elem, nodal=None, other=None)`` (the dict of
    :meth:`stress.StressRecovery.error`), ``history(traj (n_dof, n_cols))`` and ``close()`` on
    :class:`stress.StressRecovery` (``order=1``, 4-node cells) or :class:`stress.QuadraticStressRecovery` (``order=2``,
    10-node cells).  Tests pass a NumPy stand-in with the same methods.  ``element`` and ``history`` hand ``material=`` and
    ``measure=`` on; only :func:`stress_finite` and :func:`estimate_finite` give them."""
    import torch

    from .stress import QuadraticStressRecovery, StressRecovery

    Recovery = QuadraticStressRecovery if order == 2 else StressRecovery

    class _Host:
        def __init__(self, points, cells, lmd, mu):
            self.rec = Recovery(points, cells, lmd, mu, device=device)

        def _dev(self, a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.rec.torch_device)

        def element(self, X, **finite):
            return {k: _host_value(v) for k, v in self.rec.element(self._dev(X), **finite).items()}

        def nodal(self, E):
            return self.rec.nodal(self._dev(E)).cpu().numpy()

        def error(self, sigma_elem, nodal=None, other=None):
            res = self.rec.error(self._dev(sigma_elem), nodal=None if nodal is None else self._dev(nodal),
                                 other=None if other is None else self._dev(other))
            return {k: v.cpu().numpy() for k, v in res.items()}

        def history(self, traj, **finite):
            return {k: _host_value(v) for k, v in self.rec.history(traj, **finite).items()}

        def close(self):
            self.rec.close()

    return _Host


def _merge_max(best, arg, val, idx):
    """Element-wise: keep (best, arg) unless val is larger, or equal with a smaller element index."""
    take = (val > best) | ((val == best) & (idx < arg))
    return np.where(take, val, best), np.where(take, idx, arg)


def _abs_volumes(points, tets):
    vol = np.abs(np.einsum("ij,ij->i", points[tets[:, 1]] - points[tets[:, 0]],
                           np.cross(points[tets[:, 2]] - points[tets[:, 0]], points[tets[:, 3]] - points[tets[:, 0]])))
    return vol / 6.0


def _resolve_columns(columns, n_cols):
    """``columns`` as indices into ``n_cols`` saved columns (negative = from the end)."""
    cols = []
    for j in columns:
        jj = int(j) + n_cols if int(j) < 0 else int(j)
        if not 0 <= jj < n_cols:
            raise ValueError(f"column {j} out of range for {n_cols} saved columns")
        cols.append(jj)
    return cols


def _zz_entry(zz, energy_total, i, centroid):
    """The Zienkiewicz-Zhu figures of row ``i`` of ``zz`` (the dict of ``error``) and of the strain energies: ``eta``,
    ``energy_norm = sqrt(2 W)``, ``relative = eta / sqrt(energy_norm^2 + eta^2)`` and the element of the largest ``eta_e^2``."""
    eta2, w2 = float(zz["eta2_total"][i]), 2.0 * float(energy_total[i])
    e = int(zz["eta2_argmax"][i])
    return {"eta": float(np.sqrt(eta2)), "energy_norm": float(np.sqrt(w2)),
            "relative": float(np.sqrt(eta2 / (w2 + eta2))) if w2 + eta2 > 0 else 0.0, "element": e,
            "eta2_max": float(zz["eta2_max"][i]), "centroid": [float(c) for c in centroid[e]]}


def _point_data(disp, nodal):
    """Point data of one column, either order: the displacement ``(3 n,)`` or ``(n, 3)``, the recovered stress ``sigma*
    (n, 6)`` and its von Mises value."""
    from .stress import VOIGT, von_mises

    pd = {f"displacement-{c}": disp.reshape(-1, 3)[:, a] for a, c in enumerate("xyz")}
    pd.update({f"sigma-{c}": nodal[:, a] for a, c in enumerate(VOIGT)})
    pd["von-mises"] = von_mises(nodal)
    return pd


def _load_recovery_tree(p, tets, nn, runs, columns):
    """What :func:`stress` and :func:`estimate` read from the artefact tree (``p``: ``PATHS`` under the output directory):
    per rank ``(local nodes, elements)`` and the owned elements' cells in local node numbers, per run in ``runs`` the
    ranks' trajectories, the number of saved columns and ``columns`` resolved against it.  Every element must be owned
    by exactly one rank, with its nodes among that rank's local nodes; every trajectory has 3 rows per local node and
    the same columns."""
    ne = len(tets)
    ranks = []  # (local nodes, elements) for r = 0, 1, ... while Rank={r}_elements.csv exists
    while os.path.exists(p["elements"].format(r=len(ranks))):
        r = len(ranks)
        ranks.append((rio.load_int_list(p["local_nodes"].format(r=r)), rio.load_int_list(p["elements"].format(r=r))))
    if not ranks:
        raise FileNotFoundError(f"no {p['elements'].format(r=0)}: run data_prepare first")
    owner = np.full(ne, -1, dtype=np.int64)
    for r, (_, elems) in enumerate(ranks):
        if elems.size and (elems.min() < 0 or elems.max() >= ne):
            raise ValueError(f"Rank={r}_elements.csv: element id out of range 0..{ne - 1}")
        u, cnt = np.unique(elems, return_counts=True)
        if (cnt > 1).any():
            raise ValueError(f"Rank={r}_elements.csv lists element {int(u[cnt > 1][0])} more than once")
        twice = owner[elems] >= 0
        if twice.any():
            e = int(elems[twice][0])
            raise ValueError(f"element {e} is owned by ranks {int(owner[e])} and {r}")
        owner[elems] = r
    if (owner < 0).any():
        missing = np.nonzero(owner < 0)[0]
        raise ValueError(f"{len(missing)} element(s) owned by no rank (first: {int(missing[0])})")
    local_cells = []
    for r, (nodes, elems) in enumerate(ranks):
        pos = np.full(nn, -1, dtype=np.int64)
        pos[nodes] = np.arange(len(nodes))
        lc = pos[tets[elems]]
        if (lc < 0).any():
            raise ValueError(f"Rank={r}: element {int(elems[(lc < 0).any(axis=1)][0])} has a node outside "
                             f"Rank={r}_local_nodes.csv")
        local_cells.append(lc)

    trajs = {}
    for run in runs:
        trajs[run] = []
        for r, (nodes, _) in enumerate(ranks):
            path = p[run].format(r=r)
            data = np.asarray(rio.load_displacement(path), dtype=np.float64)
            if data.ndim != 2 or data.shape[0] != 3 * len(nodes):
                raise ValueError(f"{path}: {data.shape[0] if data.ndim else 0} rows, expected 3 * {len(nodes)} = "
                                 f"{3 * len(nodes)} (3 per local node)")
            trajs[run].append(data)
    n_cols = trajs["truth"][0].shape[1]
    for run in runs:
        for r, data in enumerate(trajs[run]):
            if data.shape[1] != n_cols:
                raise ValueError(f"{p[run].format(r=r)}: {data.shape[1]} saved columns, rank 0 has {n_cols}")
    return ranks, local_cells, trajs, n_cols, _resolve_columns(columns, n_cols)


def _tree_setup(mesh, out_dir, columns, modeled, device, E, nu, recovery):
    """What :func:`stress` and :func:`estimate` open with: the recovery factory with the Lame constants bound
    (``make(points, cells)``), the mesh's points and cells, ``PATHS`` under ``out_dir`` and :func:`_load_recovery_tree` of
    the synchronised run (``truth``) and, with ``modeled``, the modelled one."""
    from . import fem_setup as fs

    lmd, mu = fs.lame(DEFAULTS["E"] if E is None else E, DEFAULTS["nu"] if nu is None else nu)
    factory = _device_recovery(device) if recovery is None else recovery
    points = np.asarray(mesh.points, dtype=np.float64)
    tets = np.asarray(mesh.tets, dtype=np.int64)
    p = {k: os.path.join(out_dir, v) for k, v in PATHS.items()}
    runs = ["truth"] + (["modeled"] if modeled else [])
    return (lambda pts, cells: factory(pts, cells, lmd, mu), points, tets, p,
            *_load_recovery_tree(p, tets, len(points), runs, columns))


def _each_rank(make, points, ranks, local_cells, trajs, visit):
    """The per-rank loop of :func:`stress` and :func:`estimate`: for every rank that owns elements one recovery on its local
    nodes and cells, and ``visit(run, rec, T, elems)`` per run with the rank's trajectory ``T`` and its element ids."""
    for r, (nodes, elems) in enumerate(ranks):
        if not len(elems):
            continue
        rec = make(points[nodes], local_cells[r])
        try:
            for run in trajs:
                visit(run, rec, trajs[run][r], elems)
        finally:
            rec.close()


def stress(mesh, out_dir=".", columns=(-1,), modeled=False, history=False, vtk=True, device=0, E=None, nu=None,
           recovery=None):
    """Stress recovery from the artefact tree of :func:`data_prepare` / :func:`online_predictor` under ``out_dir``, on
    one GPU.  Each element's stress comes from the trajectory of the rank that owns it (``Rank={r}_elements.csv``,
    local dofs through ``Rank={r}_local_nodes.csv``); nodal averages are taken on the whole mesh from the assembled
    element field.  For every saved column in ``columns`` (negative = from the end) writes
    ``Results/Stress/Stress-col-{j}.vtk`` (and ``Modeled_Stress-col-{j}.vtk`` with ``modeled``) unless ``vtk`` is
    False; ``history`` writes every column's strain energy and von Mises maximum to ``Results/Stress/history.npz``.
    Returns the report that the CLI prints as JSON.  ``recovery``: see :func:`_device_recovery` (default: the GPU)."""
    from .stress import VOIGT

    make, points, tets, p, ranks, local_cells, trajs, n_cols, cols = _tree_setup(mesh, out_dir, columns, modeled, device, E,
                                                                                 nu, recovery)
    ne, nn, m, runs = len(tets), len(points), len(cols), list(trajs)

    def extremes(n):
        return dict(total=np.zeros(n), vmax=np.full(n, -np.inf), arg=np.full(n, -1, dtype=np.int64))

    fields = {run: dict(sigma=np.zeros((m, ne, 6)), von_mises=np.zeros((m, ne)), energy=np.zeros((m, ne)), **extremes(m))
              for run in runs}
    hist = {run: extremes(n_cols) for run in runs}

    def merge(f, res, elems):  # a rank's energy and von Mises maximum into those of the whole mesh
        f["total"] += res["energy_total"]
        f["vmax"], f["arg"] = _merge_max(f["vmax"], f["arg"], res["von_mises_max"],
                                         elems[np.asarray(res["von_mises_argmax"], dtype=np.int64)])

    def visit(run, rec, T, elems):
        if m:
            res = rec.element(np.ascontiguousarray(T[:, cols].T))
            for k in ("sigma", "von_mises", "energy"):
                fields[run][k][:, elems] = res[k]
            merge(fields[run], res, elems)
        if history:
            merge(hist[run], rec.history(T), elems)

    _each_rank(make, points, ranks, local_cells, trajs, visit)

    centroid = points[tets].mean(axis=1)
    interface = np.isin(tets, rio.load_int_list(p["global_shared"])).any(axis=1) if modeled else None

    def summary(f, i):
        e = int(f["arg"][i])
        return {"strain_energy": float(f["total"][i]), "von_mises_max": float(f["vmax"][i]), "element": e,
                "centroid": [float(c) for c in centroid[e]]}

    report = {"n_elems": ne, "n_nodes": nn, "n_ranks": len(ranks), "n_saved": n_cols, "columns": [], "files": [],
              "history": None}
    for i, j in enumerate(cols):
        entry = {"column": j, **summary(fields["truth"], i)}
        if modeled:
            vt, vmod = fields["truth"]["von_mises"][i], fields["modeled"]["von_mises"][i]
            dvm = np.abs(vmod - vt)
            nt = float(np.linalg.norm(vt))
            k = int(np.argmax(dvm))
            entry["modeled"] = summary(fields["modeled"], i)
            entry.update({"von_mises_rel_l2": float(np.linalg.norm(vmod - vt)) / nt if nt > 0 else float(np.linalg.norm(dvm)),
                          "dvm_max": float(dvm[k]), "dvm_element": k,
                          "dvm_max_interface": float(dvm[interface].max()) if interface.any() else 0.0,
                          "dvm_max_interior": float(dvm[~interface].max()) if (~interface).any() else 0.0})
        report["columns"].append(entry)

    if vtk and m:
        vol = _abs_volumes(points, tets)
        whole = make(points, tets)
        try:
            nodal = {run: whole.nodal(fields[run]["sigma"]) for run in runs}
        finally:
            whole.close()
        for run in runs:
            disp = np.zeros((m, nn, 3))
            for r in reversed(range(len(ranks))):  # a node held by several ranks shows the lowest rank's value
                disp[:, ranks[r][0]] = trajs[run][r][:, cols].T.reshape(m, -1, 3)
            for i, j in enumerate(cols):
                f = fields[run]
                cd = {f"sigma-{c}": f["sigma"][i, :, a] for a, c in enumerate(VOIGT)}
                cd["von-mises"] = f["von_mises"][i]
                cd["energy-density"] = np.divide(f["energy"][i], vol, out=np.zeros(ne), where=vol > 0)
                key = "stress_vtk" if run == "truth" else "modeled_stress_vtk"
                report["files"].append(rio.write_vtk_fields(p[key].format(j=j), points, tets,
                                                            _point_data(disp[i], nodal[run][i]), cd,
                                                            title=f"stress, saved column {j} ({run})"))
    if history:
        out = {"columns": np.arange(n_cols)}
        for run in runs:
            pre = "" if run == "truth" else "modeled_"
            out.update({pre + "strain_energy": hist[run]["total"], pre + "von_mises_max": hist[run]["vmax"],
                        pre + "von_mises_element": hist[run]["arg"]})
        os.makedirs(os.path.dirname(p["stress_history"]), exist_ok=True)
        np.savez(p["stress_history"], **out)
        report["history"] = p["stress_history"]
    return report


def estimate(mesh, out_dir=".", columns=(-1,), modeled=False, vtk=True, device=0, E=None, nu=None, recovery=None):
    """Zienkiewicz-Zhu estimate of the stress error of the mesh, from the artefact tree that :func:`stress` reads and with
    its ownership rule: each element's stress comes from the trajectory of the rank that owns it; the nodal average and
    ``eta_e^2 = integral_e (sigma* - sigma_e)^T D^-1 (sigma* - sigma_e) dV`` are taken on the whole mesh.  For every saved
    column in ``columns`` reports ``eta = sqrt(sum_e eta_e^2)``, ``energy_norm = sqrt(2 * strain energy)``, ``relative =
    eta / sqrt(energy_norm^2 + eta^2)`` and the element of the largest ``eta_e^2``.  With ``modeled`` also the estimate of
    the modelled run, ``model_error = sqrt(sum_e |V_e| dsigma^T D^-1 dsigma)`` (``dsigma``: modelled minus synchronised
    element stress), its ratio to ``eta``, both squared sums over interface elements (those with a ``Global_shared`` node)
    and the others, and how many elements of each set have a model error above their own ``eta_e^2``.  Writes
    ``Results/Stress/Estimate-col-{j}.vtk`` (cell data ``eta2``, ``error-density = eta2 / |V_e|`` and, with ``modeled``,
    ``model-error2``) unless ``vtk`` is False.  Returns the report that the CLI prints as JSON.  ``recovery``: see
    :func:`_device_recovery` (default: the GPU)."""
    make, points, tets, p, ranks, local_cells, trajs, n_cols, cols = _tree_setup(mesh, out_dir, columns, modeled, device, E,
                                                                                 nu, recovery)
    ne, nn, m, runs = len(tets), len(points), len(cols), list(trajs)

    sigma = {run: np.zeros((m, ne, 6)) for run in runs}
    energy = {run: np.zeros(m) for run in runs}

    def visit(run, rec, T, elems):
        res = rec.element(np.ascontiguousarray(T[:, cols].T))
        sigma[run][:, elems] = res["sigma"]
        energy[run] += res["energy_total"]

    zz, model = {}, None
    if m:
        _each_rank(make, points, ranks, local_cells, trajs, visit)
        whole = make(points, tets)
        try:
            for run in runs:
                zz[run] = whole.error(sigma[run], nodal=whole.nodal(sigma[run]))
            if modeled:
                model = whole.error(sigma["modeled"], other=sigma["truth"])
        finally:
            whole.close()

    centroid = points[tets].mean(axis=1)
    interface = np.isin(tets, rio.load_int_list(p["global_shared"])).any(axis=1) if modeled else None

    report = {"n_elems": ne, "n_nodes": nn, "n_ranks": len(ranks), "n_saved": n_cols, "columns": [], "files": []}
    for i, j in enumerate(cols):
        entry = {"column": j, **_zz_entry(zz["truth"], energy["truth"], i, centroid)}
        if modeled:
            eta2, me2 = zz["truth"]["eta2"][i], model["eta2"][i]
            above = me2 > eta2
            entry["modeled"] = _zz_entry(zz["modeled"], energy["modeled"], i, centroid)
            entry.update({"model_error": float(np.sqrt(model["eta2_total"][i])),
                          "model_over_discretisation": float(np.sqrt(model["eta2_total"][i])) / entry["eta"]
                          if entry["eta"] > 0 else None,
                          "eta2_interface": float(eta2[interface].sum()), "eta2_interior": float(eta2[~interface].sum()),
                          "model_error2_interface": float(me2[interface].sum()),
                          "model_error2_interior": float(me2[~interface].sum()),
                          "n_interface": int(interface.sum()), "n_interior": int((~interface).sum()),
                          "n_model_above_eta_interface": int((above & interface).sum()),
                          "n_model_above_eta_interior": int((above & ~interface).sum())})
        report["columns"].append(entry)

    if vtk and m:
        vol = _abs_volumes(points, tets)
        for i, j in enumerate(cols):
            eta2 = zz["truth"]["eta2"][i]
            cd = {"eta2": eta2, "error-density": np.divide(eta2, vol, out=np.zeros(ne), where=vol > 0)}
            if modeled:
                cd["model-error2"] = model["eta2"][i]
            report["files"].append(rio.write_vtk_fields(p["estimate_vtk"].format(j=j), points, tets, None, cd,
                                                        title=f"stress error estimate, saved column {j}"))
    return report


def _whole_setup(mesh, out_dir, columns, order, material, measure, device, E, nu, recovery):
    """What the whole-mesh drivers open with.  ``make()`` builds the recovery of ``order`` on the mesh (``recovery``, or the
    GPU's).  The run of ``dynamics --order {order}``: the mesh's points and its 4- or 10-node cells (order 2: elevated like
    ``dynamics --order 2``), the trajectory ``Results/Dynamics/Displacement_order{order}.hdf5`` under ``out_dir`` with 3 rows
    per node, and ``columns`` resolved against its saved columns.  ``kernels``: the keywords of ``element`` and ``history``,
    none for ``material = "linear"`` - the linear kernels take neither ``material`` nor ``measure``.  ``path(key, j=...)``: the
    entry ``key + "_p2"`` (linear) or ``key + "_fs"`` of ``PATHS`` under ``out_dir``.  The report up to ``files``; ``material``
    and ``measure`` are in it only at finite strain."""
    from . import fem_setup as fs

    lmd, mu = fs.lame(DEFAULTS["E"] if E is None else E, DEFAULTS["nu"] if nu is None else nu)
    factory = _device_recovery(device, order) if recovery is None else recovery
    if order == 2:
        mesh = _quadratic(mesh)
    points = np.asarray(mesh.points, dtype=np.float64)
    cells = np.asarray(mesh.tets10 if order == 2 else mesh.tets, dtype=np.int64)
    path = os.path.join(out_dir, PATHS["dynamics"].format(p=order))
    try:
        traj = np.asarray(rio.load_displacement(path), dtype=np.float64)
    except FileNotFoundError as exc:
        raise FileNotFoundError(f"{exc}: run dynamics --order {order} first") from None
    if traj.ndim != 2 or traj.shape[0] != 3 * len(points):
        raise ValueError(f"{path}: {traj.shape[0] if traj.ndim else 0} rows, expected 3 * {len(points)} = {3 * len(points)} "
                         + ("(3 per node of the elevated mesh)" if order == 2 else "(3 per node)"))
    cols = _resolve_columns(columns, traj.shape[1])
    finite = material != "linear"
    kernels = {"material": material, "measure": measure} if finite else {}
    key, names = ("_fs", {"material": material, "p": order}) if finite else ("_p2", {})
    report = {"order": order, "n_elems": len(cells), "n_nodes": len(points), "n_ranks": 1, "n_saved": traj.shape[1],
              **({"material": material, "measure": str(measure)} if finite else {}), "columns": [], "files": []}
    return (lambda: factory(points, cells, lmd, mu), points, cells, traj, cols, kernels,
            lambda k, **j: os.path.join(out_dir, PATHS[k + key]).format(**names, **j), report)


def _finite_material(material, order):
    """The material's name as :func:`stress_finite` and :func:`estimate_finite` report it; they refuse an ``order`` that is
    not 1 or 2 and the linear material."""
    from ._lib import material_id

    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    if material_id(material) == 0:
        raise ValueError("stress_finite / estimate_finite are for svk and neo_hookean; the linear material has stress, "
                         "stress_p2, estimate and estimate_p2")
    return str(material).replace("-", "_")


def _cell_data(res, i, finite):
    """Cell data of one column: the largest point von Mises and ``W_e`` of every element, at finite strain also its smallest
    ``det F``."""
    ne = len(res["energy"][i])
    cd ={"von-mises-max": np.asarray(res["von_mises"][i]).reshape(ne, -1).max(axis=1), "energy": res["energy"][i]}
    if finite:
        cd["det-f-min"] = np.asarray(res["det_f"][i]).reshape(ne, -1).min(axis=1)
    return cd


def _finite_figures(res, i, measure):
    """What a column's entry holds at finite strain next to the material: the measure, the inverted elements, the smallest
    ``det F``."""
    return {"measure": measure, "n_inverted": int(res["n_inverted"][i]), "min_det_f": float(np.min(res["det_f"][i]))}


def _whole_stress(mesh, out_dir, columns, order, material, measure, history, vtk, device, E, nu, recovery):
    """The whole-mesh stress driver behind :func:`stress_p2` (order 2, ``material = "linear"``: the linear kernels, which
    are given neither ``material`` nor ``measure``) and :func:`stress_finite` (either order, the material's name).  Linear
    elements with the linear material are :func:`stress`'s, on the partitioned tree."""
    from .Tools.Qudrature import Gauss_Legendre
    from .Tools.Shape_function_Deriv import Shape_Function

    make, points, cells, traj, cols, kernels, path, report = _whole_setup(mesh, out_dir, columns, order, material, measure,
                                                                          device, E, nu, recovery)
    finite, nq = material != "linear", 4 if order == 2 else 1
    # (4, 10): N_a at the Gauss points
    shape4 = np.array([Shape_Function(2, x) for x in Gauss_Legendre(2)[0]]) if order == 2 else None
    centroid = points[cells[:, :4]].mean(axis=1)
    report["history"] = None
    rec = make()
    try:
        if cols:
            X = np.ascontiguousarray(traj[:, cols].T)
            res = rec.element(X, **kernels)
            nodal = rec.nodal(res["sigma"]) if vtk else None
            for i, j in enumerate(cols):
                e, q = divmod(int(res["von_mises_argmax"][i]), nq)
                entry = {"column": j, "strain_energy": float(res["energy_total"][i]),
                         "von_mises_max": float(res["von_mises_max"][i]), "element": e}
                if order == 2:
                    entry.update({"gauss_point": q, "position": [float(c) for c in shape4[q] @ points[cells[e]]]})
                entry["centroid"] = [float(c) for c in centroid[e]]
                if finite:
                    entry.update({**_finite_figures(res, i, res["measure"]), "material": material})
                report["columns"].append(entry)
                if vtk:
                    title = f"{measure} stress, {material}, order {order}" if finite else "stress, quadratic tetrahedra"
                    report["files"].append(rio.write_vtk_fields(path("stress_vtk", j=j), points, cells,
                                                                _point_data(X[i], nodal[i]), _cell_data(res, i, finite),
                                                                title=f"{title}, saved column {j}"))
        if history:
            h = rec.history(traj, **kernels)
            arg = np.asarray(h["von_mises_argmax"], dtype=np.int64)
            out = dict(columns=np.arange(traj.shape[1]), strain_energy=h["energy_total"], von_mises_max=h["von_mises_max"],
                       von_mises_element=arg // nq, von_mises_gauss_point=arg % nq)
            if finite:
                out.update(n_inverted=h["n_inverted"], min_det_f=h["min_det_f"])
            report["history"] = path("stress_history")
            os.makedirs(os.path.dirname(report["history"]), exist_ok=True)
            np.savez(report["history"], **out)
    finally:
        rec.close()
    return report


def _whole_estimate(mesh, out_dir, columns, order, material, vtk, device, E, nu, recovery):
    """The whole-mesh estimate driver behind :func:`estimate_p2` (order 2, ``material = "linear"``) and
    :func:`estimate_finite` (either order, the material's name: the second Piola-Kirchhoff stress), on the run and with the
    rules of :func:`_whole_stress`."""
    make, points, cells, traj, cols, kernels, path, report = _whole_setup(mesh, out_dir, columns, order, material, "pk2",
                                                                          device, E, nu, recovery)
    finite = material != "linear"
    centroid = points[cells[:, :4]].mean(axis=1)
    if not cols:
        return report
    rec = make()
    try:
        X = np.ascontiguousarray(traj[:, cols].T)
        res = rec.element(X, **kernels)
        nodal = rec.nodal(res["sigma"])
        zz = rec.error(res["sigma"], nodal=nodal)
    finally:
        rec.close()
    for i, j in enumerate(cols):
        entry = {"column": j, **_zz_entry(zz, res["energy_total"], i, centroid)}
        if finite:
            entry.update({"material": material, **_finite_figures(res, i, "pk2")})
        report["columns"].append(entry)
        if vtk:
            title = f"{material}, order {order}" if finite else "quadratic tetrahedra"
            report["files"].append(rio.write_vtk_fields(path("estimate_vtk", j=j), points, cells, _point_data(X[i], nodal[i]),
                                                        {**_cell_data(res, i, finite), "eta2": zz["eta2"][i]},
                                                        title=f"stress error estimate, {title}, saved column {j}"))
    return report


def stress_p2(mesh, out_dir=".", columns=(-1,), history=False, vtk=True, device=0, E=None, nu=None, recovery=None):
    """:func:`stress` for quadratic tetrahedra: the whole mesh on one GPU, the displacement of ``dynamics --order 2``
    (``Results/Dynamics/Displacement_order2.hdf5`` under ``out_dir``).  For every saved column in ``columns`` reports the
    strain energy, the largest Gauss-point von Mises stress, its element, Gauss point and position, and writes
    ``Results/Stress/Stress-order2-col-{j}.vtk`` (type-24 cells; point data: displacement, the recovered stress ``sigma*``
    and its von Mises; cell data: the largest Gauss-point von Mises and ``W_e``) unless ``vtk`` is False; ``history`` writes
    every column's strain energy and von Mises maximum to ``Results/Stress/history-order2.npz``.  Returns the report that
    the CLI prints as JSON.  ``recovery``: see :func:`_device_recovery` of order 2 (default: the GPU)."""
    return _whole_stress(mesh, out_dir, columns, 2, "linear", None, history, vtk, device, E, nu, recovery)


def estimate_p2(mesh, out_dir=".", columns=(-1,), vtk=True, device=0, E=None, nu=None, recovery=None):
    """:func:`estimate` for quadratic tetrahedra, on the run that :func:`stress_p2` reads: the Zienkiewicz-Zhu estimate
    ``eta_e^2 = integral_e (sigma* - sigma_h)^T D^-1 (sigma* - sigma_h) dV`` with the element-linear stress ``sigma_h`` and
    the quadratic field ``sigma*`` of its recovered nodal values.  For every saved column in ``columns`` reports ``eta``,
    ``energy_norm``, ``relative`` and the element of the largest ``eta_e^2`` with its centroid, and writes
    ``Results/Stress/Estimate-order2-col-{j}.vtk`` (type-24 cells; point data as :func:`stress_p2`; cell data: the largest
    Gauss-point von Mises, ``W_e`` and ``eta2``) unless ``vtk`` is False.  ``recovery``: see :func:`_device_recovery`."""
    return _whole_estimate(mesh, out_dir, columns, 2, "linear", vtk, device, E, nu, recovery)


def stress_finite(mesh, out_dir=".", columns=(-1,), material="svk", measure="cauchy", order=1, history=False, vtk=True,
                  device=0, E=None, nu=None, recovery=None):
    """:func:`stress` at finite strain (``material``: ``svk`` or ``neo_hookean``; ``measure``: ``cauchy`` or ``pk2``), for
    either element order: the whole mesh on one GPU, the displacement of ``dynamics --order {order} --material ...``
    (``Results/Dynamics/Displacement_order{order}.hdf5`` under ``out_dir``).  For every saved column in ``columns`` reports
    the stored energy (``strain_energy``), the largest point von Mises stress of ``measure`` with its element (order 2: Gauss
    point and position too), the number of inverted elements and the smallest ``det F``, and writes
    ``Results/Stress/Stress-{material}-order{order}-col-{j}.vtk`` (point data: displacement, the recovered stress and its von
    Mises; cell data: the largest point von Mises, ``W_e`` and the smallest ``det F``) unless ``vtk`` is False; ``history``
    writes every column's stored energy, von Mises maximum, inverted count and smallest ``det F`` to
    ``Results/Stress/history-{material}-order{order}.npz``.  There is no modelled finite-strain run.  Returns the report that
    the CLI prints as JSON.  ``recovery``: see :func:`_device_recovery` of that order (default: the GPU)."""
    return _whole_stress(mesh, out_dir, columns, order, _finite_material(material, order), measure, history, vtk, device, E,
                         nu, recovery)


def estimate_finite(mesh, out_dir=".", columns=(-1,), material="svk", order=1, vtk=True, device=0, E=None, nu=None,
                    recovery=None):
    """:func:`estimate` at finite strain, on the run that :func:`stress_finite` reads, always with the second
    Piola-Kirchhoff stress over the reference configuration: ``eta_e^2 = integral_0 (S* - S_h)^T D^-1 (S* - S_h) dV`` with
    the recovered nodal field ``S*`` (the kernels of the linear estimate of that order).  For ``svk`` this is exactly the
    energy norm of the Green-strain error; for ``neo_hookean`` ``D`` is the linearised material and ``eta`` a scale in its
    norm.  For every saved column in ``columns`` reports ``eta``, ``energy_norm = sqrt(2 * stored energy)``, ``relative`` and
    the element of the largest ``eta_e^2`` with its centroid, ``n_inverted`` and ``min_det_f``, and writes
    ``Results/Stress/Estimate-{material}-order{order}-col-{j}.vtk`` (point data as :func:`stress_finite`, of PK2; cell data:
    the largest point von Mises, ``W_e``, the smallest ``det F`` and ``eta2``) unless ``vtk`` is False."""
    return _whole_estimate(mesh, out_dir, columns, order, _finite_material(material, order), vtk, device, E, nu, recovery)


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def _load_mesh(args):
    return structured_beam(args.synthetic) if args.synthetic else read_vtk(args.mesh)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="synchronization_avoiding_algorithms_amd.drivers")
    ap.add_argument("command", choices=["data_prepare", "steady_state", "shared_extraction", "model_training",
                                        "online_predictor", "modal", "stress", "estimate", "dynamics"])
    ap.add_argument("--epochs", type=int, default=None, help="model_training: override the epoch count")
    ap.add_argument("--mesh", default="Mesh_info/beam_coarse.vtk")
    ap.add_argument("--synthetic", type=int, default=0, help="use the 25n x n x n synthetic beam instead")
    ap.add_argument("--steps", type=int, default=100000)      # test_num, Data_prepare.py:49
    ap.add_argument("--save-every", type=int, default=1)      # Data_prepare.py:50
    ap.add_argument("--out", default=".")
    ap.add_argument("--partition", choices=["slab", "graph", "rcb"], default="slab")
    ap.add_argument("--parts", type=int, default=0,
                    help="dynamics: cut the mesh into this many parts and run them as ranks of a partition on one GPU")
    ap.add_argument("--energy", action="store_true",
                    help="dynamics: record the energy balance (kinetic, strain, work, damping loss) and store the table")
    ap.add_argument("--energy-every", type=int, default=1, help="dynamics --energy: every so many steps")
    ap.add_argument("--material", choices=["linear", "svk", "neo-hookean"], default="linear",
                    help="dynamics: the element pass - small-strain linear elasticity, or finite strain with the St. "
                         "Venant-Kirchhoff or the compressible neo-Hookean material.  dt stays gamma * 2/omega_max of the linear "
                         "operator at the reference configuration: under large stretch the stability limit moves and the "
                         "stepper does not follow it unless --dt-follow asks for it.  stress, estimate: the finite-strain stress of that material on the "
                         "whole-mesh run of dynamics (either order)")
    ap.add_argument("--measure", choices=["cauchy", "pk2"], default="cauchy",
                    help="stress --material svk / neo-hookean: the Cauchy or the second Piola-Kirchhoff stress (estimate "
                         "always uses pk2)")
    ap.add_argument("--fz", type=float, default=0.5,
                    help="dynamics, steady_state --material, modal --material: the amplitude of the load (0, -fz, -fz); at the "
                         "default nothing is nonlinear")
    ap.add_argument("--load-steps", type=int, default=1,
                    help="steady_state, modal --material svk / neo-hookean: apply the load in this many equal fractions")
    ap.add_argument("--fx", type=float, default=0.0,
                    help="modal --material svk / neo-hookean: the axial part of the load (fx, -fz, -fz); negative compresses "
                         "the beam")
    ap.add_argument("--dt-check-every", type=int, default=0,
                    help="dynamics --material svk / neo-hookean: every so many steps measure 2/omega_max of the tangent at the "
                         "current state and report it against dt (dt_check); dt is not changed")
    ap.add_argument("--dt-follow", choices=["certified", "anchored"], default=None,
                    help="dynamics --material svk / neo-hookean: follow the stable step - before step 0 and after every "
                         "--dt-follow-every steps bound omega_max of the tangent at the current state in one element pass and "
                         "change dt exactly.  certified: gamma * 2/bound (safe, pessimistic); anchored: the linear operator's "
                         "step scaled by bound(0)/bound(state) (a heuristic, never above today's dt)")
    ap.add_argument("--dt-follow-every", type=int, default=10, help="dynamics --dt-follow: every so many steps")
    ap.add_argument("--scheme", choices=["explicit", "newmark"], default="explicit",
                    help="dynamics: explicit central differences (dt = gamma * 2/omega_max), or implicit Newmark (the trapezoidal "
                         "rule; a Newton iteration per step with a Jacobi-PCG on the device) at dt = --dt-factor * 2/omega_max")
    ap.add_argument("--dt-factor", type=float, default=10.0,
                    help="dynamics --scheme newmark: dt as a multiple of the explicit limit 2/omega_max of the linear operator")
    ap.add_argument("--newton-tol", type=float, default=1e-10,
                    help="dynamics --scheme newmark: a step has converged at |r| <= tol * max(|load|, |f_int|, |inertia + damping|)")
    ap.add_argument("--n-past", type=int, default=20)
    ap.add_argument("--n-future", type=int, default=20)
    ap.add_argument("--filter-size", type=int, default=150)
    ap.add_argument("--hidden-size", type=int, default=50)
    ap.add_argument("--resync-every", type=int, default=None,
                    help="online_predictor: synchronised steps again after every so many predicted windows (extension; "
                         "default: never, like the reference)")
    ap.add_argument("--resync-steps", type=int, default=None, help="how many (default: one window, n_future*filter_size)")
    ap.add_argument("--delaunay", action="store_true",
                    help="modal, stress, estimate: the unstructured delaunay_beam(n) for --synthetic n")
    ap.add_argument("--k", type=int, default=6, help="modal: number of lowest modes")
    ap.add_argument("--columns", default="-1", help="stress, estimate: saved columns, comma-separated, negative from the end")
    ap.add_argument("--modeled", action="store_true", help="stress, estimate: the modelled run too, and its differences")
    ap.add_argument("--history", action="store_true", help="stress: every column's strain energy and von Mises maximum")
    ap.add_argument("--no-vtk", action="store_true", help="stress, estimate: no VTK files")
    ap.add_argument("--order", type=int, choices=[1, 2], default=1,
                    help="steady_state, modal, dynamics, stress, estimate: 2 = quadratic tetrahedra (the mesh is elevated "
                         "unless the file holds tetra10); stress and estimate then read the run of dynamics --order 2")
    args = ap.parse_args(argv)
    if args.command == "dynamics" and args.scheme == "newmark":
        if args.parts and args.parts > 0:
            ap.error("dynamics --scheme newmark --parts: the implicit stepper runs the whole mesh (no partitions)")
        if args.energy:
            ap.error("dynamics --scheme newmark --energy: the implicit stepper records no energy table")
        if args.dt_follow:
            ap.error("dynamics --scheme newmark --dt-follow: the implicit step is not tied to the stability limit")
        if args.dt_check_every:
            ap.error("dynamics --scheme newmark --dt-check-every: the implicit step is not tied to the stability limit")
        if not (args.dt_factor > 0 and args.newton_tol > 0):
            ap.error("dynamics --scheme newmark: --dt-factor and --newton-tol must be > 0")
    if args.command == "dynamics" and args.energy and args.material != "linear":
        ap.error(f"dynamics --material {args.material} --energy: the energy balance is defined for the linear material only "
                 "(its identity needs a symmetric constant K)")
    if args.command == "dynamics" and args.dt_check_every:
        if args.dt_check_every < 0:
            ap.error("dynamics --dt-check-every must be >= 0")
        if args.material == "linear":
            ap.error("dynamics --dt-check-every: the check is for --material svk or neo-hookean (the linear operator's limit "
                     "does not move)")
        if args.parts and args.parts > 0:
            ap.error("dynamics --dt-check-every --parts: a rank's operator is only its share of the tangent; run the check "
                     "on the whole mesh")
    if args.command == "dynamics" and args.dt_follow:
        if args.dt_follow_every < 1:
            ap.error("dynamics --dt-follow-every must be >= 1")
        if args.material == "linear":
            ap.error("dynamics --dt-follow: following the step is for --material svk or neo-hookean (the linear operator's limit "
                     "does not move)")
        if args.parts and args.parts > 0:
            ap.error("dynamics --dt-follow --parts: a rank holds only its share of the internal force; follow the step on the "
                     "whole mesh")
        if args.energy:
            ap.error("dynamics --dt-follow --energy: the identity of the energy balance assumes one dt")
    if args.command == "steady_state" and args.load_steps < 1:
        ap.error("steady_state --load-steps must be >= 1")
    if args.command == "modal" and args.load_steps < 1:
        ap.error("modal --load-steps must be >= 1")
    if args.command == "modal" and args.material == "linear" and args.fx != 0.0:
        ap.error("modal --fx: the prestress is for --material svk or neo-hookean (a linear operator's modes do not depend on "
                 "the load)")
    if args.command in ("stress", "estimate") and args.material != "linear" and args.modeled:
        ap.error(f"{args.command} --material {args.material} --modeled: there is no modelled finite-strain run (the predictor "
                 "drives the linear material)")
    if args.command in ("stress", "estimate") and args.order == 2 and args.modeled:
        ap.error(f"{args.command} --order 2 --modeled: there is no modelled p = 2 run (the predictor drives linear elements)")
    rank, world, local = _dist_env()
    if args.command in ("modal", "stress", "estimate", "dynamics"):  # one whole mesh on one GPU; prints one JSON object
        if rank != 0:
            return
        import json

        from .mesh import delaunay_beam

        mesh = (delaunay_beam(args.synthetic) if args.delaunay else structured_beam(args.synthetic)) if args.synthetic \
            else read_vtk(args.mesh)
        if args.command == "modal":
            extra = {} if args.material == "linear" else {"material": args.material, "fz": args.fz, "fx": args.fx,
                                                          "load_steps": args.load_steps}
            print(json.dumps(modal(mesh, k=args.k, device=local, order=args.order, **extra)))
        elif args.command == "dynamics":
            path, report = dynamics(mesh, args.steps, args.save_every, args.out, device=local, order=args.order,
                                    parts=args.parts, partition=args.partition,
                                    energy_every=max(args.energy_every, 1) if args.energy else 0, fz=args.fz,
                                    material=args.material, dt_check_every=args.dt_check_every, dt_follow=args.dt_follow,
                                    dt_follow_every=args.dt_follow_every,
                                    **({"scheme": "newmark", "dt_factor": args.dt_factor, "newton_tol": args.newton_tol}
                                       if args.scheme == "newmark" else {}))
            print(json.dumps({**report, "path": path}))
        else:  # stress, estimate: the driver of (material, order); only stress has a history and a choice of measure
            only_stress = args.command == "stress"
            kw = {"vtk": not args.no_vtk, "device": local, **({"history": args.history} if only_stress else {})}
            if args.material != "linear":
                driver = stress_finite if only_stress else estimate_finite
                kw.update({"material": args.material, "order": args.order, **({"measure": args.measure} if only_stress else {})})
            elif args.order == 2:
                driver = stress_p2 if only_stress else estimate_p2
            else:
                driver = stress if only_stress else estimate
                kw["modeled"] = args.modeled
            print(json.dumps(driver(mesh, args.out, [int(c) for c in args.columns.split(",") if c.strip()], **kw)))
        return
    if args.command == "data_prepare":
        path, _ = data_prepare(_load_mesh(args), args.steps, args.save_every, args.out, rank, world,
                               args.partition, device=local, verbose=True)
    elif args.command == "steady_state":
        if rank != 0:
            return
        if args.material != "linear":
            import json

            try:
                path, _, report = steady_state_nonlinear(_load_mesh(args), args.out, device=local, material=args.material,
                                                         order=args.order, fz=args.fz, load_steps=args.load_steps)
            except NotConverged as exc:
                print(json.dumps(exc.report))
                raise SystemExit(f"error: {exc}") from None
            print(json.dumps({**report, "path": path}))
            return
        path, _ = steady_state(_load_mesh(args), args.out, device=local, verbose=True, order=args.order)
    elif args.command == "shared_extraction":
        path, _ = shared_extraction(args.out, rank)
    elif args.command == "model_training":
        from .training import train_rank_model

        path, _, _ = train_rank_model(args.out, rank, device=f"cuda:{local}" if _has_gpu() else "cpu",
                                      hidden_size=args.hidden_size, filter_size=args.filter_size,
                                      n_past=args.n_past, n_future=args.n_future, num_epochs=args.epochs,
                                      verbose=True)
    else:
        path, _, _ = online_predictor(_load_mesh(args), args.steps, args.save_every, args.out, rank, world,
                                      args.partition, device=local, n_past=args.n_past, n_future=args.n_future,
                                      filter_size=args.filter_size, hidden_size=args.hidden_size,
                                      resync_every=args.resync_every, resync_steps=args.resync_steps)
    print(f"[rank {rank}] wrote {path}")


if __name__ == "__main__":
    main()
