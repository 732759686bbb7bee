"""Steady state ``K d = F`` on the GPU, matrix-free.

The reference solves it once before the time stepping, on rank 0, with a dense ``np.linalg.solve`` on the
``(3N)^2`` matrix of ``Global_Assembly`` (/root/reference ``Tools/Steady_solvers.py:13-22``, called at
``Data_prepare.py:157-168`` with the un-ramped load) and writes ``Results/Static/steady_distributed.vtk``.
Here: Jacobi-preconditioned conjugate gradients whose operator is the FORCE_ONLY kernel of the time stepper
(``saa_internal_force_device``), all vectors resident on the GPU as float64 torch tensors; Dirichlet dofs are
eliminated the way ``Global_Assembly`` does it (rows and columns dropped, ``Mat_construction.py:176-192``).
"""
from __future__ import annotations

import numpy as np


def stiffness_diagonal(points, cells, lmd, mu) -> np.ndarray:
    """diag(K) of the linear-tet stiffness, ``(3N,)``: ``V (lambda g_A^2 + mu (|g|^2 + g_A^2))`` per node ``a`` and
    component ``A`` of every element, ``g = grad N_a`` (closed form of ``Local_K_coronary``,
    ``Mat_construction.py:79-119``)."""
    p = np.asarray(points, dtype=np.float64)[np.asarray(cells)]
    e1, e2, e3 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]
    c1, c2, c3 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
    det = np.einsum("ij,ij->i", e1, c1)
    g = np.stack([-(c1 + c2 + c3), c1, c2, c3], axis=1) / det[:, None, None]          # (Ne, 4, 3)
    vol = (det / 6.0)[:, None, None]
    diag_e = vol * (lmd * g ** 2 + mu * ((g ** 2).sum(axis=2, keepdims=True) + g ** 2))  # (Ne, 4, 3)
    dof = 3 * np.asarray(cells)[:, :, None] + np.arange(3)[None, None, :]
    return np.bincount(dof.ravel(), weights=diag_e.ravel(), minlength=3 * len(points))


def steady_solve(solver, f_ext, dirichlet_dofs, diag=None, tol=1e-12, max_iter=None, check_every=25, device=None):
    """Solve ``K d = f_ext`` with ``d[dirichlet_dofs] = 0`` -> ``(d (3n,1) numpy, iterations, relative residual)``.

    ``solver``: a :class:`HipExplicitSolver` (caller numbering); ``diag``: optional ``diag(K)`` for the Jacobi
    preconditioner (:func:`stiffness_diagonal`).  Converged when ``|r| <= tol |b|``.
    """
    import torch

    dev = torch.device("cuda", solver.device if device is None else device)
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    n = solver.n_dof
    free = torch.ones(n, dtype=torch.float64, device=dev)
    if len(dirichlet_dofs):
        free[torch.as_tensor(np.asarray(dirichlet_dofs, dtype=np.int64), device=dev)] = 0.0
    b = torch.as_tensor(np.asarray(f_ext, dtype=np.float64).reshape(-1), device=dev) * free
    minv = free.clone()
    if diag is not None:
        dk = torch.as_tensor(np.asarray(diag, dtype=np.float64).reshape(-1), device=dev)
        minv = torch.where(dk > 0, free / dk, free)
    x = torch.zeros_like(b)
    r = b.clone()
    z = minv * r
    p = z.clone()
    ap = torch.empty_like(b)
    rz = torch.dot(r, z)
    bnorm = float(torch.linalg.vector_norm(b))
    if bnorm == 0.0:
        return np.zeros((n, 1)), 0, 0.0
    max_iter = max_iter or 20 * n
    it, rel = 0, 1.0
    while it < max_iter:
        solver.internal_force_device(p, ap)      # K p on the GPU (no matrix anywhere)
        ap.mul_(free)
        alpha = rz / torch.dot(p, ap)
        x.add_(alpha * p)
        r.sub_(alpha * ap)
        z = minv * r
        rz_new = torch.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
        if it % check_every == 0:                # the only host synchronisation
            rel = float(torch.linalg.vector_norm(r)) / bnorm
            if rel <= tol:
                break
    rel = float(torch.linalg.vector_norm(r)) / bnorm
    return x.cpu().numpy().reshape(-1, 1), it, rel


def steady_solve_operator(op, b, tol=1e-12, max_iter=None, check_every=25):
    """Jacobi-PCG for ``K d = b`` on an operator handle (:class:`modal.ModalOperator`) of either order, for one right-hand
    side ``(n_dof,)`` or several ``(m, n_dof)`` (float64 tensors on the operator's device, or arrays).  The loop of
    :func:`steady_solve`, one independent iteration per right-hand side batched through the block apply and
    preconditioned with ``op.diagonal()``; Dirichlet dofs are eliminated by the operator's mask.  A right-hand side is
    converged when ``|r| <= tol |b|``.  Returns ``(d, iterations, relative residual)``: ``d`` a NumPy array of the shape
    of ``b``, the residual that of the iteration as :func:`steady_solve` reports it, the largest over the right-hand
    sides."""
    import torch

    B = b if torch.is_tensor(b) else torch.as_tensor(np.asarray(b, dtype=np.float64))
    B = B.to(device=op.torch_device, dtype=torch.float64)
    vec = B.dim() == 1
    B = B.reshape(-1, op.n_dof) * op.free
    diag_k, _ = op.diagonal(k=True, m=False)
    minv = torch.where(diag_k > 0, op.free / torch.where(diag_k > 0, diag_k, 1.0), op.free)
    X = torch.zeros_like(B)
    bnorm = torch.linalg.vector_norm(B, dim=1)
    live = bnorm > 0
    safe = torch.where(live, bnorm, 1.0)
    R = B.clone()
    Z = minv * R
    P = Z.clone()
    rz = (R * Z).sum(dim=1)
    max_iter = max_iter or 20 * op.n_dof
    it = 0
    running = bool(live.any())
    while it < max_iter and running:
        AP = op.apply(P)[0]
        pap = (P * AP).sum(dim=1)
        ok = live & (pap > 0)
        alpha = torch.where(ok, rz / torch.where(ok, pap, 1.0), 0.0)
        X += alpha[:, None] * P
        R -= alpha[:, None] * AP
        Z = minv * R
        rz_new = (R * Z).sum(dim=1)
        beta = torch.where(rz > 0, rz_new / torch.where(rz > 0, rz, 1.0), 0.0)
        P = Z + beta[:, None] * P
        rz = rz_new
        it += 1
        if it % check_every == 0:                # the only host synchronisation
            live = live & (torch.linalg.vector_norm(R, dim=1) > tol * bnorm)
            running = bool(live.any())
    rel = float((torch.linalg.vector_norm(R, dim=1) / safe).max())
    d = X.cpu().numpy()
    return (d[0] if vec else d), it, rel


def _tangent_pcg(apply_kt, r0, minv, rtol, max_iter, check_every):
    """The Jacobi-PCG loop of :func:`steady_solve_operator` on one right-hand side ``r0`` with the operator ``apply_kt`` (a
    tangent, which need not be positive definite), from 0 until ``|r| <= rtol |r0|``.  It stops at the first direction with
    ``p . K_T p <= 0`` and returns the iterate so far, or the preconditioned residual ``minv r0`` when it has made no step.
    The curvature test stays on the device; the host looks every ``check_every`` iterations.  ``(x, iterations)``."""
    import torch

    x = torch.zeros_like(r0)
    r = r0.clone()
    z = minv * r
    z0 = z
    p = z.clone()
    rz = torch.dot(r, z)
    target = rtol * float(torch.linalg.vector_norm(r0))
    alive = torch.ones((), dtype=torch.float64, device=r0.device)
    steps = torch.zeros((), dtype=torch.float64, device=r0.device)
    it = 0
    while it < max_iter:
        ap = apply_kt(p)
        pap = torch.dot(p, ap)
        alive = alive * (pap > 0)
        alpha = alive * rz / torch.where(pap > 0, pap, 1.0)
        x = x + alpha * p
        r = r - alpha * ap
        steps = steps + alive
        z = minv * r
        rz_new = torch.dot(r, z)
        p = z + torch.where(rz > 0, rz_new / torch.where(rz > 0, rz, 1.0), 0.0) * p
        rz = rz_new
        it += 1
        if it % check_every == 0 or it == 1:     # the only host synchronisations (the first: a start without curvature)
            if float(alive) == 0.0 or float(torch.linalg.vector_norm(r)) <= target:
                break
    return (x if float(steps) > 0 else z0), it


def newton_solve_operator(op, b, material, u0=None, tol=1e-10, max_newton=50, load_steps=1, check_every=25):
    """The static equilibrium ``f_int(u) = b`` of a finite-strain material (``svk``, ``neo_hookean``) on an operator handle
    (:class:`modal.ModalOperator`) of either order: ``|f_int(u) - b| <= tol |b|`` on the free dofs, ``u = 0`` on the others.

    Per load fraction ``k / load_steps`` an inexact Newton iteration (at most ``max_newton`` each): the system ``K_T(u) du =
    b_k - f_int(u)`` by the Jacobi-PCG loop of :func:`steady_solve_operator` on ``op.tangent_apply``, preconditioned with
    ``op.diagonal()`` of the linear ``K``, to a forcing tolerance that shrinks with the residual (Eisenstat-Walker's second
    choice, ``0.9 (|r_k| / |r_k-1|)^2`` in ``[tol-limited floor, 0.1]``); CG stops at the first ``p . K_T p <= 0`` and hands
    back the iterate so far, or the preconditioned residual if it has none.  Then a backtracking Armijo line search on ``Pi(u)
    - b_k . u`` with ``Pi`` the sum of ``energy_elem`` of ``op.internal_force(..., energy=True)``; a trial in which neo-Hooke
    finds an inverted element is rejected like an increase.  Two energies closer than their round-off (``8 eps (|Pi| + |b .
    u|)``) count as equal, since near the solution the decrease is of the order of the residual squared.  Intermediate load
    fractions are solved to ``max(tol, 1e-6)`` only: they are starting points.  The iteration also ends, unconverged, when
    three steps in a row were accepted inside that round-off without lowering the residual: ``f_int`` is then at its own
    round-off, which on a slender beam is far above ``eps`` - the nodal displacements are mostly rigid motion of the element
    (``eps (L/h)^4`` of ``|b|``, about 1e-9 on a 25 : 1 cantilever).

    Returns ``(u (n_dof,) NumPy, info)``; ``info``: ``converged``, ``newton_iterations``, ``cg_iterations``, ``residual`` (``|f_int(u)
    - b| / |b|`` recomputed with ``internal_force`` at the end), ``residual_history`` (one per Newton iteration, relative to the
    full ``|b|``), ``load_steps``, ``n_inverted`` (at the returned ``u``).  It does not raise when it does not converge."""
    import torch

    from . import _lib

    if _lib.material_id(material) == 0:
        raise ValueError("newton_solve_operator is for svk and neo_hookean; the linear solve is steady_solve_operator")
    if int(load_steps) < 1:
        raise ValueError("load_steps must be >= 1")
    B = b if torch.is_tensor(b) else torch.as_tensor(np.asarray(b, dtype=np.float64))
    B = B.to(device=op.torch_device, dtype=torch.float64).reshape(-1) * op.free
    if B.numel() != op.n_dof:
        raise ValueError(f"b must hold {op.n_dof} values")
    if u0 is None:
        u = torch.zeros_like(B)
    else:
        u = u0 if torch.is_tensor(u0) else torch.as_tensor(np.asarray(u0, dtype=np.float64))
        u = u.to(device=op.torch_device, dtype=torch.float64).reshape(-1) * op.free
    diag_k, _ = op.diagonal(k=True, m=False)
    minv = torch.where(diag_k > 0, op.free / torch.where(diag_k > 0, diag_k, 1.0), op.free)
    bnorm = float(torch.linalg.vector_norm(B))
    info = {"converged": True, "newton_iterations": 0, "cg_iterations": 0, "residual": 0.0, "residual_history": [],
            "load_steps": int(load_steps), "n_inverted": 0}
    if bnorm == 0.0 and u0 is None:
        return np.zeros(op.n_dof), info
    scale = bnorm if bnorm > 0 else 1.0
    eps = float(np.finfo(np.float64).eps)
    max_cg = 20 * op.n_dof

    def state(x, bk):
        f, en, n_inv = op.internal_force(x, material, energy=True)
        pi, work = float(en.sum()), float(torch.dot(bk, x))
        return (bk - f) * op.free, pi - work, 8.0 * eps * (abs(pi) + abs(work)), n_inv

    for k in range(1, int(load_steps) + 1):
        bk = B * (k / int(load_steps))
        goal = (tol if k == int(load_steps) else max(tol, 1e-6)) * scale
        r, phi, noise, n_inv = state(u, bk)
        rnorm, previous, done, stalled = float(torch.linalg.vector_norm(r)), None, False, 0
        for _ in range(int(max_newton)):
            if rnorm <= goal:
                done = True
                break
            eta = 0.1 if previous is None else min(0.1, 0.9 * (rnorm / previous) ** 2)
            eta = max(eta, 0.1 * goal / rnorm)
            du, its = _tangent_pcg(lambda p: op.tangent_apply(u, p, material), r, minv, eta, max_cg, check_every)
            info["cg_iterations"] += its
            slope = -float(torch.dot(r, du))
            if not slope < 0.0:                  # not a descent direction: steepest descent in the preconditioner's metric
                du = minv * r
                slope = -float(torch.dot(r, du))
            t, accepted = 1.0, None
            for _ in range(40):
                trial = u + t * du
                rt, phit, noiset, inv_t = state(trial, bk)
                if inv_t == 0 and phit <= phi + 1e-4 * t * slope + max(noise, noiset):
                    accepted = (trial, rt, phit, noiset, inv_t)
                    in_noise = phit > phi + 1e-4 * t * slope
                    break
                t *= 0.5
            info["newton_iterations"] += 1
            if accepted is None:
                break
            previous = rnorm
            u, r, phi, noise, n_inv = accepted
            rnorm = float(torch.linalg.vector_norm(r))
            info["residual_history"].append(rnorm / scale)
            stalled = stalled + 1 if in_noise and rnorm >= previous else 0
            if stalled >= 3:                     # the residual sits at the round-off of f_int: no step can lower it
                break
        else:
            done = rnorm <= goal
        if not done:
            info["converged"] = False
            break
    f, _, n_inv = op.internal_force(u, material, energy=True)
    info["residual"] = float(torch.linalg.vector_norm((B - f) * op.free)) / scale
    info["n_inverted"] = int(n_inv)
    info["converged"] = bool(info["converged"] and info["residual"] <= tol and n_inv == 0)
    return u.cpu().numpy(), info


def write_vtk_point_data(path, points, cells, displacement, extra=None):
    """Legacy-VTK file with the mesh and the point data ``displacement-x/-y/-z`` - the arrays the reference hands to
    ``meshio.write_points_cells`` at ``Data_prepare.py:165-168`` (ASCII here).  4-column cells are written as VTK type 10,
    10-column cells (quadratic tetrahedra) as type 24.  ``extra``: further point scalars ``{name: (n,) array}``, written
    after the displacement, which stays what it is without them."""
    import os

    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells)
    d = np.asarray(displacement, dtype=np.float64).reshape(-1, 3)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("# vtk DataFile Version 4.2\nsteady solution d = K^-1 F\nASCII\nDATASET UNSTRUCTURED_GRID\n")
        fh.write(f"POINTS {len(points)} double\n")
        np.savetxt(fh, points, fmt="%.17g")
        width = cells.shape[1] if cells.ndim == 2 else 4
        fh.write(f"CELLS {len(cells)} {(width + 1) * len(cells)}\n")
        np.savetxt(fh, np.column_stack([np.full(len(cells), width), cells]), fmt="%d")
        fh.write(f"CELL_TYPES {len(cells)}\n")
        np.savetxt(fh, np.full(len(cells), 24 if width == 10 else 10), fmt="%d")
        fh.write(f"POINT_DATA {len(points)}\n")
        for c, name in enumerate(("displacement-x", "displacement-y", "displacement-z")):
            fh.write(f"SCALARS {name} double 1\nLOOKUP_TABLE default\n")
            np.savetxt(fh, d[:, c], fmt="%.17g")
        for name, a in (extra or {}).items():
            fh.write(f"SCALARS {name} double 1\nLOOKUP_TABLE default\n")
            np.savetxt(fh, np.asarray(a, dtype=np.float64).reshape(len(points)), fmt="%.17g")
    return path
