"""Modal analysis on the GPU: the stable time step of the explicit solver and the lowest natural frequencies.

The central-difference update of ``Tools/Dynamic_solver.py:13-20`` is stable only if ``dt < 2/omega_max``, with
``omega_max`` the largest eigenfrequency of ``M_L^-1 K`` on the free dofs (``M_L`` the lumped mass of
``commons.py:103-107``).  The reference never computes it: its ``dt`` comes from the edge-length rule
(``commons.py:79-90``, ``Data_prepare.py:147``), here ``fem_setup.dt_from_min_edge``.  This module reports three figures:

* ``dt_reference`` - that rule, unchanged (what every driver, test and bench still uses);
* ``dt_crit = 2/omega_max`` - the sharp limit, from Lanczos on ``M_L^-1/2 K M_L^-1/2`` (:func:`lanczos_max`);
* ``dt_bound = 2/max_e omega_e`` - a safe lower bound from the element kernel (Irons-Treharne: ``omega_max <= max_e
  omega_e``, ``omega_e^2 = lambda_max(K_e)/(rho |V_e|/4)``), valid ("certified") only when every signed volume is > 0.

Damping does not move the limit.  The reference's update is mass-proportional: per mode of ``M_L^-1 K`` (eigenvalue
``omega^2``) it reads ``(1+a) z^2 - (2-x) z + (1-a) = 0`` with ``a = alpha dt/2`` and ``x = (omega dt)^2``.  For
``alpha >= 0`` the product of the roots ``(1-a)/(1+a)`` has modulus below 1, and the Jury conditions ``p(1) = x > 0``
and ``p(-1) = 4 - x > 0`` leave ``0 <= x < 4``, i.e. ``omega dt < 2``, whatever ``alpha``.  So ``2/omega_max`` is the
limit of this solver with the reference's ``alpha = 0.5`` too.

The lowest modes (:func:`lowest_modes`) solve ``K x = omega^2 M x`` with the consistent mass ``M`` (the pair of the
reference's ``Eigen_mode``, ``Tools/Steady_solvers.py:25-40``) by block shift-invert subspace iteration at sigma = 0,
whose inner solves are Jacobi-preconditioned CG on the block apply (``steady.steady_solve`` for several right-hand sides
at once).  Both solvers are written against plain callables on float64 torch tensors, so that they run on the CPU
against assembled matrices as well as on the GPU against :class:`ModalOperator`.  Blocks of vectors are ``(m, n)``
tensors, one vector per row (column-major ``n x m`` in memory, what ``saa_operator_apply`` reads).
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import _lib


# ------------------------------------------------------------------------------------------------------------------
# Element stable frequencies, host restatement (the kernel's formula in NumPy)
# ------------------------------------------------------------------------------------------------------------------

def elasticity_cholesky(lmd, mu) -> np.ndarray:
    """``L`` with ``D = L L^T``, ``D`` the isotropic 6x6 matrix of ``commons.py:25-31`` (Voigt xx,yy,zz,yz,xz,xy)."""
    D = np.zeros((6, 6))
    D[:3, :3] = lmd
    D[np.arange(3), np.arange(3)] = lmd + 2.0 * mu
    D[np.arange(3, 6), np.arange(3, 6)] = mu
    return np.linalg.cholesky(D)


def element_omega(points, cells, lmd, mu, rho):
    """``(omega_e, signed volume)`` per element: ``omega_e^2 = (4/rho) lambda_max(B^T D B)`` taken from the 6x6
    ``L^T (B B^T) L`` (same nonzero spectrum as the 12x12 ``B^T D B``), what ``saa_operator_element_bound`` computes."""
    p = np.asarray(points, dtype=np.float64)[np.asarray(cells)]
    e1, e2, e3 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]
    c = np.stack([np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)], axis=1)
    det = np.einsum("ij,ij->i", e1, c[:, 0])
    g = c / det[:, None, None]
    g = np.concatenate([-g.sum(axis=1, keepdims=True), g], axis=1)                      # (ne, 4, 3) grad N_a
    S = np.einsum("eai,eaj->eij", g, g)
    sxx, syy, szz, sxy, sxz, syz = S[:, 0, 0], S[:, 1, 1], S[:, 2, 2], S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]
    z = np.zeros_like(sxx)
    G = np.stack([np.stack(r, axis=1) for r in (
        (sxx, z, z, z, sxz, sxy), (z, syy, z, syz, z, sxy), (z, z, szz, syz, sxz, z),
        (z, syz, syz, syy + szz, sxy, sxz), (sxz, z, sxz, sxy, sxx + szz, syz), (sxy, sxy, z, sxz, syz, sxx + syy))],
        axis=1)                                                                           # (ne, 6, 6) = B B^T
    L = elasticity_cholesky(lmd, mu)
    A = np.einsum("ki,ekl,lj->eij", L, G, L)
    lam = np.linalg.eigvalsh(A)[:, -1]
    return np.sqrt(4.0 / rho * lam), det / 6.0


# ------------------------------------------------------------------------------------------------------------------
# The device operator
# ------------------------------------------------------------------------------------------------------------------

class ModalOperator:
    """One ``saa_operator`` handle: the whole mesh on one GPU in the caller's numbering, the stiffness / consistent-mass
    block apply with Dirichlet masking, and the element stable-frequency bound.  float64 CUDA tensors in and out.

    ``cells`` of shape ``(ne, 10)`` (``mesh.to_quadratic``) make an order-2 handle (``saa_operator_create_p2``): quadratic
    tetrahedra, ``K`` with the reference's 4-point rule, ``M`` with the 14-point rule.  ``apply``, ``load`` and
    ``diagonal`` work on either order; ``element_bound`` and the linear stress recovery (:class:`stress.StressRecovery`)
    are linear-element formulas and raise on an order-2 handle, whose stress comes from
    :class:`stress.QuadraticStressRecovery`."""

    MAX_COLUMNS = 16

    def __init__(self, points, cells, dirichlet_dofs, lmd, mu, rho, device=0):
        import torch

        self._lib = _lib.load()
        self._h = C.c_void_p()
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1))
        cells = np.asarray(cells, dtype=np.int32)
        per_elem = 10 if cells.ndim == 2 and cells.shape[1] == 10 else 4
        tets = np.ascontiguousarray(cells.reshape(-1))
        dd = np.ascontiguousarray(np.asarray(dirichlet_dofs, dtype=np.int32).reshape(-1))
        self.n_nodes, self.n_elems = pts.size // 3, tets.size // per_elem
        self.n_dof = 3 * self.n_nodes
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        create = self._lib.saa_operator_create_p2 if per_elem == 10 else self._lib.saa_operator_create
        _lib.check(create(
            self.device, self.n_nodes, self.n_elems, pts.ctypes.data_as(dp), tets.ctypes.data_as(ip) if tets.size else None,
            dd.ctypes.data_as(ip) if dd.size else None, int(dd.size), float(lmd), float(mu), float(rho), C.byref(self._h)))
        free = torch.ones(self.n_dof, dtype=torch.float64, device=self.torch_device)
        if dd.size:
            free[torch.as_tensor(dd.astype(np.int64), device=self.torch_device)] = 0.0
        self.free = free
        self.order = int(self._lib.saa_operator_order(self._h))
        self.set_stream(torch.cuda.current_stream(self.torch_device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.saa_operator_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, stream_ptr):
        _lib.check(self._lib.saa_operator_set_stream(self._h, C.c_void_p(int(stream_ptr) if stream_ptr else 0)))

    def apply_raw(self, m, x, ldx, kx=None, mx=None, ldy=None):
        """One ``saa_operator_apply`` call on raw device pointers (``m`` may be anything: the library checks it)."""
        _lib.check(self._lib.saa_operator_apply(self._h, int(m), C.c_void_p(x.data_ptr()), int(ldx),
                                                C.c_void_p(kx.data_ptr()) if kx is not None else None,
                                                C.c_void_p(mx.data_ptr()) if mx is not None else None,
                                                int(ldx if ldy is None else ldy)))

    def apply(self, x, k=True, m=False):
        """``(K x, M x)`` (either None when not asked for) of a ``(n_dof,)`` vector or an ``(m, n_dof)`` block, in as
        many launches of at most 16 columns as it takes."""
        import torch

        if not (x.is_cuda and x.dtype == torch.float64):
            raise ValueError("x must be a float64 CUDA tensor")
        vec = x.dim() == 1
        X = x.reshape(1, -1) if vec else x
        if X.shape[1] != self.n_dof:
            raise ValueError(f"expected {self.n_dof} dofs per vector, got {X.shape[1]}")
        X = X.contiguous()
        KX = torch.empty_like(X) if k else None
        MX = torch.empty_like(X) if m else None
        for j in range(0, X.shape[0], self.MAX_COLUMNS):
            c = min(self.MAX_COLUMNS, X.shape[0] - j)
            self.apply_raw(c, X[j], self.n_dof, KX[j] if k else None, MX[j] if m else None)
        if vec:
            return (KX.reshape(-1) if k else None), (MX.reshape(-1) if m else None)
        return KX, MX

    def load(self, f):
        """The consistent body-force vector of the force density ``f = (fx, fy, fz)`` (``Fe`` of ``Local_MKF`` assembled,
        0 on Dirichlet dofs) as an ``(n_dof,)`` CUDA tensor."""
        import torch

        fx, fy, fz = (float(c) for c in np.asarray(f, dtype=np.float64).reshape(-1))
        out = torch.empty(self.n_dof, dtype=torch.float64, device=self.torch_device)
        _lib.check(self._lib.saa_operator_load(self._h, fx, fy, fz, C.c_void_p(out.data_ptr())))
        return out

    def diagonal(self, k=True, m=True):
        """``(diag K, diag M)`` of the masked operator (0 on Dirichlet dofs; either None when not asked for)."""
        import torch

        dk = torch.empty(self.n_dof, dtype=torch.float64, device=self.torch_device) if k else None
        dm = torch.empty(self.n_dof, dtype=torch.float64, device=self.torch_device) if m else None
        _lib.check(self._lib.saa_operator_diagonal(self._h, C.c_void_p(dk.data_ptr()) if k else None,
                                                   C.c_void_p(dm.data_ptr()) if m else None))
        return dk, dm

    def lumped_mass(self):
        """The lumped mass as an ``(n_dof,)`` CUDA tensor, one value on a node's three dofs, Dirichlet dofs included
        (``saa_operator_lumped_mass``).  Order 2: HRZ lumping with the 14-point rule (the reference's row sum gives every
        vertex of a quadratic tetrahedron a negative mass); order 1: the row sum ``rho V/4``."""
        import torch

        out = torch.empty(self.n_dof, dtype=torch.float64, device=self.torch_device)
        _lib.check(self._lib.saa_operator_lumped_mass(self._h, C.c_void_p(out.data_ptr())))
        return out

    def internal_force(self, x, material="svk", energy=False):
        """The internal force ``f_int(x)`` of one ``(n_dof,)`` float64 CUDA displacement vector under ``material``
        (``linear``, ``svk``: St. Venant-Kirchhoff, ``neo_hookean``: compressible neo-Hooke; ``include/saa_hip.h`` has the
        definitions), 0 on Dirichlet dofs (``saa_operator_internal_force``).  ``linear`` is ``apply(x)[0]`` bit for bit.
        ``energy=True`` (not with ``linear``): returns ``(f, energy_elem, n_inverted)`` - the stored energy per element and
        the number of elements that neo-Hooke found inverted (``!(det F > 0)`` at a point), which contributed 0."""
        import torch

        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.numel() == self.n_dof):
            raise ValueError(f"x must be a float64 CUDA tensor of {self.n_dof} values")
        x = x.reshape(-1).contiguous()
        f = torch.empty_like(x)
        en = torch.empty(self.n_elems, dtype=torch.float64, device=self.torch_device) if energy else None
        n_inv = C.c_int64(0)
        _lib.check(self._lib.saa_operator_internal_force(self._h, _lib.material_id(material), C.c_void_p(x.data_ptr()),
                                                         C.c_void_p(f.data_ptr()), C.c_void_p(en.data_ptr()) if energy else None,
                                                         C.byref(n_inv) if energy else None))
        return (f, en, int(n_inv.value)) if energy else f

    def tangent_apply(self, u, v, material="svk", count=False):
        """``K_T(u) v``, the tangent of :meth:`internal_force` at the displacement ``u`` applied to ``v`` (both ``(n_dof,)``
        float64 CUDA tensors, masked on Dirichlet dofs on input), 0 on Dirichlet dofs (``saa_operator_tangent_apply``).
        ``linear`` is ``apply(v)[0]`` bit for bit and ``u`` may then be None.  ``count=True``: returns ``(kv, n_inverted)`` -
        the number of elements that neo-Hooke found inverted at ``u``, which contributed 0 - and synchronises."""
        import torch

        def ok(x):
            return torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.numel() == self.n_dof

        mat = _lib.material_id(material)
        if not ok(v):
            raise ValueError(f"v must be a float64 CUDA tensor of {self.n_dof} values")
        if not (ok(u) or (u is None and mat == 0)):
            raise ValueError(f"u must be a float64 CUDA tensor of {self.n_dof} values")
        v = v.reshape(-1).contiguous()
        u = u.reshape(-1).contiguous() if u is not None else None
        kv = torch.empty_like(v)
        n_inv = C.c_int64(0)
        _lib.check(self._lib.saa_operator_tangent_apply(self._h, mat, C.c_void_p(u.data_ptr()) if u is not None else None,
                                                        C.c_void_p(v.data_ptr()), C.c_void_p(kv.data_ptr()),
                                                        C.byref(n_inv) if count else None))
        return (kv, int(n_inv.value)) if count else kv

    def shifted_apply(self, u, v, shift, material="svk", dot=False):
        """``K_T(u) v + shift * v`` (``saa_operator_shifted_apply``), 0 on Dirichlet dofs: the operator of an implicit step, with
        ``shift`` a diagonal such as ``(4/dt^2 + 2 alpha/dt) m``.  ``u``, ``v``, ``shift``: ``(n_dof,)`` float64 CUDA tensors, ``u``
        and ``v`` masked on Dirichlet dofs on input; ``u`` may be None with ``linear``.  ``shift=None`` is :meth:`tangent_apply` bit
        for bit.  ``dot=True``: returns ``(out, v . out)``, the product a 0-dim CUDA tensor summed on the device in a fixed order
        (no synchronisation)."""
        import torch

        def ok(x):
            return torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.numel() == self.n_dof

        mat = _lib.material_id(material)
        if not ok(v):
            raise ValueError(f"v must be a float64 CUDA tensor of {self.n_dof} values")
        if not (ok(u) or (u is None and mat == 0)):
            raise ValueError(f"u must be a float64 CUDA tensor of {self.n_dof} values")
        if not (shift is None or ok(shift)):
            raise ValueError(f"shift must be None or a float64 CUDA tensor of {self.n_dof} values")
        v = v.reshape(-1).contiguous()
        u = u.reshape(-1).contiguous() if u is not None else None
        shift = shift.reshape(-1).contiguous() if shift is not None else None
        out = torch.empty_like(v)
        prod = torch.zeros((), dtype=torch.float64, device=v.device) if dot else None
        _lib.check(self._lib.saa_operator_shifted_apply(self._h, mat, C.c_void_p(u.data_ptr()) if u is not None else None,
                                                        C.c_void_p(v.data_ptr()),
                                                        C.c_void_p(shift.data_ptr()) if shift is not None else None,
                                                        C.c_void_p(out.data_ptr()), C.c_void_p(prod.data_ptr()) if dot else None,
                                                        None))
        return (out, prod) if dot else out

    def tangent_apply_block(self, u, V, material="svk", count=False):
        """``K_T(u) v`` for every row ``v`` of the ``(m, n_dof)`` float64 CUDA block ``V`` (or one ``(n_dof,)`` vector), in as
        many ``saa_operator_tangent_apply_block`` calls of at most 16 columns as it takes: what does not depend on the column
        is done once per call.  A row's result does not depend on the rows next to it.  ``linear`` is ``apply(V)[0]`` bit for
        bit and ``u`` may then be None.  ``count=True``: returns ``(KV, n_inverted)`` - the number of elements that neo-Hooke
        found inverted at ``u`` (the same in every call; elements, not elements times columns) - and synchronises."""
        import torch

        mat = _lib.material_id(material)
        if not (torch.is_tensor(V) and V.is_cuda and V.dtype == torch.float64 and V.dim() in (1, 2)):
            raise ValueError("V must be a float64 CUDA tensor, (m, n_dof) or (n_dof,)")
        vec = V.dim() == 1
        X = (V.reshape(1, -1) if vec else V).contiguous()
        if X.shape[1] != self.n_dof:
            raise ValueError(f"expected {self.n_dof} dofs per vector, got {X.shape[1]}")
        if u is None:
            if mat != 0:
                raise ValueError("a nonlinear material needs the state at which its tangent is taken")
        elif not (torch.is_tensor(u) and u.is_cuda and u.dtype == torch.float64 and u.numel() == self.n_dof):
            raise ValueError(f"u must be a float64 CUDA tensor of {self.n_dof} values")
        u = u.reshape(-1).contiguous() if u is not None else None
        KX = torch.empty_like(X)
        n_inv, worst = C.c_int64(0), 0
        for j in range(0, X.shape[0], self.MAX_COLUMNS):
            c = min(self.MAX_COLUMNS, X.shape[0] - j)
            _lib.check(self._lib.saa_operator_tangent_apply_block(
                self._h, mat, C.c_void_p(u.data_ptr()) if u is not None else None, c, C.c_void_p(X[j].data_ptr()), self.n_dof,
                C.c_void_p(KX[j].data_ptr()), self.n_dof, C.byref(n_inv) if count else None))
            worst = max(worst, int(n_inv.value))
        KX = KX.reshape(-1) if vec else KX
        return (KX, worst) if count else KX

    def element_bound(self, return_omega=False) -> dict:
        """``omega_max`` bound ``max_e omega_e``, its element, the count of elements with signed volume <= 0 and
        whether the bound is certified (that count is 0); ``omega_e`` (a CUDA tensor) on request."""
        import torch

        om = torch.empty(self.n_elems, dtype=torch.float64, device=self.torch_device) if return_omega else None
        wmax, arg, nneg = C.c_double(), C.c_int32(), C.c_int32()
        _lib.check(self._lib.saa_operator_element_bound(self._h, C.c_void_p(om.data_ptr()) if om is not None else None,
                                                        C.byref(wmax), C.byref(arg), C.byref(nneg)))
        out = {"omega_max": wmax.value, "element": arg.value, "n_nonpositive": nneg.value, "certified": nneg.value == 0}
        if return_omega:
            out["omega_e"] = om
        return out

    def tangent_bound(self, u, material="svk", return_omega=False) -> dict:
        """An upper bound of ``omega_max`` of ``M_L^-1 K_T(u)`` from one element pass (``saa_operator_tangent_bound``, either
        order): ``omega_max = max_e omega_e`` and its ``element`` (ties: the lowest index; 0 and -1 when no element enters the
        maximum), ``n_nonpositive`` (elements with ``detJ <= 0`` at a point: the bound is ``certified`` only when 0),
        ``n_inverted`` (neo-Hooke elements with ``!(J > 0)`` at a point: ``omega_e = 0``, left out of the maximum) and
        ``n_nonfinite`` (elements whose ``omega_e`` is not finite: left out and counted); ``omega_e`` (a CUDA tensor) on request.
        ``u``: an ``(n_dof,)`` float64 CUDA tensor, masked on Dirichlet dofs on input; None with ``linear``, whose operator does
        not depend on it.  A bound, not an estimate: ``include/saa_hip.h`` has the definition.  Synchronises."""
        import torch

        mat = _lib.material_id(material)
        if u is None:
            if mat != 0:
                raise ValueError("a nonlinear material needs the state at which its tangent is taken")
        elif not (torch.is_tensor(u) and u.is_cuda and u.dtype == torch.float64 and u.numel() == self.n_dof):
            raise ValueError(f"u must be a float64 CUDA tensor of {self.n_dof} values")
        u = u.reshape(-1).contiguous() if u is not None else None
        om = torch.empty(self.n_elems, dtype=torch.float64, device=self.torch_device) if return_omega else None
        wmax, arg, counts = C.c_double(), C.c_int32(), (C.c_int64 * 3)()
        _lib.check(self._lib.saa_operator_tangent_bound(self._h, mat, C.c_void_p(u.data_ptr()) if u is not None else None,
                                                        C.c_void_p(om.data_ptr()) if om is not None else None, C.byref(wmax),
                                                        C.byref(arg), counts))
        out = {"omega_max": wmax.value, "element": arg.value, "n_nonpositive": int(counts[0]), "n_inverted": int(counts[1]),
               "n_nonfinite": int(counts[2]), "certified": int(counts[0]) == 0}
        if return_omega:
            out["omega_e"] = om
        return out


# ------------------------------------------------------------------------------------------------------------------
# Solvers on plain callables
# ------------------------------------------------------------------------------------------------------------------

def lanczos_max(apply_k, inv_sqrt_mass, max_iter=300, tol=1e-10, check_every=10, seed=0):
    """Largest eigenvalue of ``A = S K S`` with ``S = diag(inv_sqrt_mass)`` (``M_L^-1/2`` on the free dofs, 0 on the
    Dirichlet dofs) by Lanczos with full reorthogonalisation.  ``apply_k``: ``(m, n) -> (m, n)`` block apply of ``K``.

    Returns ``(omega_max, residual, iterations)`` with ``omega_max = sqrt(theta)`` of the top Ritz value and
    ``residual = |A y - theta y| / theta`` of its Ritz vector, computed with one extra apply (not estimated).  Stops once
    the Lanczos estimate of that residual is below ``tol`` or after ``max_iter`` steps."""
    import torch
    from scipy.linalg import eigh_tridiagonal

    s = inv_sqrt_mass
    n = s.numel()

    def A(v):
        return s * apply_k((s * v).reshape(1, -1)).reshape(-1)

    g = torch.Generator(device="cpu").manual_seed(seed)
    q = (torch.rand(n, generator=g, dtype=torch.float64) - 0.5).to(s.device) * (s != 0)
    q = q / torch.linalg.vector_norm(q)
    max_iter = min(max_iter, int((s != 0).sum()))
    Q = torch.zeros((max_iter + 1, n), dtype=torch.float64, device=s.device)
    Q[0] = q
    alpha, beta = [], []
    theta, svec, it = 0.0, None, 0
    for j in range(max_iter):
        w = A(Q[j])
        a = torch.dot(Q[j], w)
        w = w - a * Q[j] - (beta[-1] * Q[j - 1] if j > 0 else 0.0)
        for _ in range(2):  # full reorthogonalisation, twice is enough
            w = w - Q[: j + 1].T @ (Q[: j + 1] @ w)
        b = float(torch.linalg.vector_norm(w))
        alpha.append(float(a))
        beta.append(b)
        it = j + 1
        last = it == max_iter or b == 0.0
        if it % check_every == 0 or last:
            ev, vec = eigh_tridiagonal(np.array(alpha), np.array(beta[:-1]))
            theta, svec = float(ev[-1]), vec[:, -1]
            if abs(b * svec[-1]) <= tol * abs(theta) or last:
                break
        Q[j + 1] = w / b
    y = torch.as_tensor(svec, dtype=torch.float64, device=s.device) @ Q[:it]
    r = A(y) - theta * y
    res = float(torch.linalg.vector_norm(r) / (abs(theta) * torch.linalg.vector_norm(y)))
    return math.sqrt(max(theta, 0.0)), res, it


def _block_pcg(apply_k, B, X, dinv, rtol, max_iter, check_every=10, curvature=None):
    """Independent Jacobi-PCG solves ``K x_i = b_i`` for the rows of ``B``, batched through the block apply, starting
    from ``X`` (updated in place).  A row stops once its residual fell by ``rtol`` from its start (or to 1e-15 |b_i|).
    Returns the number of iterations.

    ``curvature`` (a dict, for an operator that may be indefinite): the first direction of each active row with ``p . K p
    <= 0`` is kept on the device (``curvature["found"]`` per row, ``["p"]``, ``["pkp"]``); the host looks at the checks it
    already makes and the loop ends there once any row has one."""
    import torch

    R = B - apply_k(X)
    r0 = torch.linalg.vector_norm(R, dim=1)
    target = torch.maximum(rtol * r0, 1e-15 * torch.linalg.vector_norm(B, dim=1))
    active = r0 > target
    if not bool(active.any()):
        return 0
    Z = dinv * R
    P = Z.clone()
    rz = (R * Z).sum(dim=1)
    if curvature is not None:
        curvature.update({"found": torch.zeros_like(active), "p": torch.zeros_like(P), "pkp": torch.zeros_like(rz)})
    it = 0
    while it < max_iter:
        AP = apply_k(P)
        pap = (P * AP).sum(dim=1)
        if curvature is not None:
            new = active & ~(pap > 0) & ~curvature["found"]
            curvature["p"] = torch.where(new[:, None], P, curvature["p"])
            curvature["pkp"] = torch.where(new, pap, curvature["pkp"])
            curvature["found"] = curvature["found"] | new
        alpha = torch.where(active & (pap > 0), rz / torch.where(pap > 0, pap, 1.0), 0.0)
        X += alpha[:, None] * P
        R -= alpha[:, None] * AP
        Z = dinv * R
        rz_new = (R * Z).sum(dim=1)
        beta = torch.where(rz > 0, rz_new / torch.where(rz > 0, rz, 1.0), 0.0)
        P = Z + beta[:, None] * P
        rz = rz_new
        it += 1
        if it % check_every == 0:
            active = active & (torch.linalg.vector_norm(R, dim=1) > target)
            if not bool(active.any()):
                break
            if curvature is not None and bool(curvature["found"].any()):
                break
    return it


def _rayleigh_ritz(Y, KY, MY):
    """Ritz pairs of ``(K, M)`` in the row space of ``Y``: ``(theta ascending, Q, KQ, MQ)``."""
    import torch
    from scipy.linalg import eigh

    nrm = torch.sqrt((Y * MY).sum(dim=1)).clamp_min(1e-300)
    Y, KY, MY = Y / nrm[:, None], KY / nrm[:, None], MY / nrm[:, None]
    Kp = (Y @ KY.T).cpu().numpy()
    Mp = (Y @ MY.T).cpu().numpy()
    Kp, Mp = 0.5 * (Kp + Kp.T), 0.5 * (Mp + Mp.T)
    try:
        theta, V = eigh(Kp, Mp)
    except np.linalg.LinAlgError:  # nearly dependent rows: drop the directions Mp cannot tell apart
        w, U = np.linalg.eigh(Mp)
        keep = w > 1e-14 * w.max()
        T = U[:, keep] / np.sqrt(w[keep])
        theta, W = np.linalg.eigh(T.T @ Kp @ T)
        V = T @ W
    Vt = torch.as_tensor(V.T.copy(), dtype=torch.float64, device=Y.device)
    return theta, Vt @ Y, Vt @ KY, Vt @ MY


def lowest_modes(apply_k, apply_m, k, free, diag_k=None, block=None, tol=1e-8, max_outer=60, inner_rtol=1e-3,
                 max_inner=20000, seed=0, indefinite=False):
    """The ``k`` lowest eigenpairs of ``K x = omega^2 M x`` on the free dofs (``free``: ``(n,)`` tensor, 1 on free dofs,
    0 on Dirichlet dofs; ``apply_k`` / ``apply_m``: ``(m, n) -> (m, n)`` block applies that return 0 on Dirichlet dofs).

    Block shift-invert subspace iteration at sigma = 0 (``K`` is SPD on the free dofs): each sweep solves
    ``K Y = M Q`` for the current Ritz vectors ``Q`` by batched Jacobi-PCG (``diag_k`` = ``diag(K)``; started from
    ``Q / theta``, which already solves it up to the Ritz residual, and stopped after a fixed reduction ``inner_rtol``),
    then a Rayleigh-Ritz step on ``(K, M)`` in the span of ``Y``.  ``block`` vectors (default ``max(2k, k+8)``) are
    iterated so that the ``k``-th converges at rate ``omega_k^2 / omega_(block+1)^2``.

    Returns a dict: ``omega2`` (ascending), ``frequencies_hz`` = ``omega/2pi``, ``residuals`` =
    ``|K x - omega^2 M x| / (omega^2 |M x|)`` per mode (computed, not estimated), ``vectors`` ``(k, n)``,
    ``outer_iterations``, ``inner_iterations`` and ``converged`` (every residual <= ``tol``).  The iteration also ends
when three sweeps in a row fail to halve the largest residual: on fine meshes round-off in ``K x`` bounds the residual
from below by about ``eps omega_max^2 / omega_i^2``, and ``converged`` then stays False.

    ``indefinite=True`` is for a ``K`` that need not be positive definite (a tangent at a loaded state,
    :func:`prestressed_modes`).  Every Rayleigh quotient ``x . K x / x . M x`` bounds the lowest eigenvalue from above, so a
    non-positive one proves that there is a non-positive eigenvalue, and shift-invert at 0 has nothing to converge to.  The
    same iteration then stops at the first proof - a Ritz value ``<= 0`` after a Rayleigh-Ritz step, or an active column of
    the inner PCG with ``p . K p <= 0`` (tested on the device, read at the checks the PCG makes anyway) - and the dict also
    holds ``stable`` (no proof was met) and ``lowest_ritz`` (stable: the lowest Ritz value; else the most negative Rayleigh
    quotient formed, finite and ``<= 0``).  An unstable result has ``converged`` False and None for ``omega2``,
    ``frequencies_hz``, ``residuals`` and ``vectors``: it claims no frequencies."""
    import torch

    def unstable(lowest):
        return {"omega2": None, "frequencies_hz": None, "residuals": None, "vectors": None, "outer_iterations": outer,
                "inner_iterations": inner, "converged": False, "stable": False, "lowest_ritz": float(lowest)}

    def inner_solve(Y):
        """The inner PCG; with ``indefinite`` also the lowest Rayleigh quotient of a direction without curvature, or None."""
        if not indefinite:
            return _block_pcg(apply_k, MQ, Y, dinv, inner_rtol, max_inner), None
        seen = {}
        its = _block_pcg(apply_k, MQ, Y, dinv, inner_rtol, max_inner, curvature=seen)
        if not seen or not bool(seen["found"].any()):
            return its, None
        pmp = (seen["p"] * apply_m(seen["p"])).sum(dim=1)
        rq = torch.where(seen["found"] & (pmp > 0), seen["pkp"] / torch.where(pmp > 0, pmp, 1.0), 0.0)
        return its, float(rq.min())

    n = free.numel()
    n_free = int((free != 0).sum())
    k = min(int(k), n_free)
    p = min(n_free, block or max(2 * k, k + 8))
    dinv = free.clone() if diag_k is None else torch.where(diag_k > 0, free / torch.where(diag_k > 0, diag_k, 1.0), free)
    g = torch.Generator(device="cpu").manual_seed(seed)
    Y = (torch.rand((p, n), generator=g, dtype=torch.float64) - 0.5).to(free.device) * free
    theta, Q, KQ, MQ = _rayleigh_ritz(Y, apply_k(Y), apply_m(Y))
    inner, outer, res, best, stalled = 0, 0, None, np.inf, 0
    if indefinite and not float(np.min(theta)) > 0.0:
        return unstable(np.min(theta))
    for outer in range(1, max_outer + 1):
        th = torch.as_tensor(theta, dtype=torch.float64, device=free.device)
        Y = Q / th.clamp_min(1e-300)[:, None]
        its, flat = inner_solve(Y)
        inner += its
        if flat is not None:
            return unstable(flat)
        theta, Q, KQ, MQ = _rayleigh_ritz(Y, apply_k(Y), apply_m(Y))
        if indefinite and not float(np.min(theta)) > 0.0:
            return unstable(np.min(theta))
        th = torch.as_tensor(theta[:k], dtype=torch.float64, device=free.device)
        R = KQ[:k] - th[:, None] * MQ[:k]
        res = (torch.linalg.vector_norm(R, dim=1) / (th.abs() * torch.linalg.vector_norm(MQ[:k], dim=1))).cpu().numpy()
        if (res <= tol).all():
            break
        # round-off floor (about eps * omega_max^2 / omega_i^2 on fine meshes): stop once three sweeps gained < 2x
        stalled = stalled + 1 if res.max() > 0.5 * best else 0
        best = min(best, float(res.max()))
        if stalled >= 3:
            break
    omega2 = np.asarray(theta[:k], dtype=np.float64)
    out = {"omega2": omega2, "frequencies_hz": np.sqrt(np.maximum(omega2, 0.0)) / (2.0 * np.pi), "residuals": res,
           "vectors": Q[:k], "outer_iterations": outer, "inner_iterations": inner, "converged": bool((res <= tol).all())}
    if indefinite:
        out.update({"stable": True, "lowest_ritz": float(np.min(theta))})
    return out


# ------------------------------------------------------------------------------------------------------------------
# Front ends
# ------------------------------------------------------------------------------------------------------------------

def _sync(device):
    import torch

    torch.cuda.synchronize(device)
    return time.perf_counter()


def stable_time_step(points, cells, dirichlet_nodes, E, nu, rho, gamma=0.9, device=0, operator=None, lanczos_tol=1e-10):
    """The three time-step figures of the explicit solver on this mesh (module docstring): ``dt_reference`` (the
    reference's rule, as the drivers evaluate it), ``dt_crit = 2/omega_max`` (Lanczos), ``dt_bound = 2/max_e omega_e``
    (element kernel), ``certified`` (every signed volume > 0, so that ``dt_bound <= dt_crit`` is guaranteed),
    ``critical_element`` (argmax of ``omega_e``) and ``ratio = dt_reference / dt_crit``."""
    import torch

    from . import fem_setup as fs

    points = np.ascontiguousarray(points, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    lmd, mu = fs.lame(E, nu)
    dev = torch.device("cuda", device)
    t0 = _sync(dev)
    lumped, _, min_edge = fs.device_setup_fields(points, cells, rho, 0.0, device)
    dt_reference = fs.dt_from_min_edge(min_edge, E, nu, rho, gamma)
    op = operator or ModalOperator(points, cells, fs.node_to_dof(dirichlet_nodes), lmd, mu, rho, device)
    try:
        t1 = _sync(dev)
        bound = op.element_bound()
        t2 = _sync(dev)
        lm = torch.as_tensor(np.asarray(lumped, dtype=np.float64).reshape(-1), device=dev)
        s = op.free / torch.sqrt(lm)
        omega_max, res, its = lanczos_max(lambda X: op.apply(X)[0], s, tol=lanczos_tol)
        t3 = _sync(dev)
    finally:
        if operator is None:
            op.close()
    dt_crit = 2.0 / omega_max
    return {"dt_reference": dt_reference, "dt_crit": dt_crit, "dt_bound": 2.0 / bound["omega_max"],
            "certified": bound["certified"], "critical_element": bound["element"], "n_nonpositive": bound["n_nonpositive"],
            "ratio": dt_reference / dt_crit, "omega_max": omega_max, "omega_bound": bound["omega_max"],
            "lanczos_residual": res, "lanczos_iterations": its,
            "seconds": {"setup": t1 - t0, "element_bound": t2 - t1, "lanczos": t3 - t2}}


def stable_time_step_operator(op: ModalOperator, mass, gamma=0.9, lanczos_tol=1e-10, material="linear", state=None) -> dict:
    """``{"omega_max", "dt_crit", "dt"}`` of the central-difference update on an operator handle of either order with the
    lumped mass ``mass`` (``(n_dof,)``, e.g. :meth:`ModalOperator.lumped_mass`): ``omega_max`` of ``M_L^-1 K`` on the free
    dofs by :func:`lanczos_max` on the handle's ``K`` apply, ``dt_crit = 2/omega_max`` and ``dt = gamma * dt_crit``.  The
    step of :class:`dynamics.OperatorStepper`; nothing else picks its ``dt`` from it.

    With a nonlinear ``material`` and a ``state`` (an ``(n_dof,)`` float64 CUDA displacement) the operator is the tangent
    ``K_T(state)`` of that material (:meth:`ModalOperator.tangent_apply`): the limit of the linearised update at that state.
    The dict then also holds ``material``, ``n_inverted`` (elements neo-Hooke dropped from the tangent) and
    ``lanczos_residual``."""
    import torch

    m = mass if torch.is_tensor(mass) else torch.as_tensor(np.asarray(mass, dtype=np.float64))
    m = m.to(device=op.torch_device, dtype=torch.float64).reshape(-1)
    s = torch.where(m > 0, op.free / torch.sqrt(torch.where(m > 0, m, 1.0)), 0.0)  # (a node without elements has no mass)
    mat = _lib.material_id(material)
    if mat == 0:
        if state is not None:
            raise ValueError("a state is given with the linear material, whose operator does not depend on it")
        omega_max, _, _ = lanczos_max(lambda X: op.apply(X)[0], s, tol=lanczos_tol)
        dt_crit = 2.0 / omega_max
        return {"omega_max": omega_max, "dt_crit": dt_crit, "dt": gamma * dt_crit}
    if state is None:
        raise ValueError("a nonlinear material needs the state at which its tangent is taken")
    state = state.reshape(-1).contiguous()
    n_inverted = op.tangent_apply(state, s, material, count=True)[1]
    omega_max, res, _ = lanczos_max(lambda X: op.tangent_apply(state, X.reshape(-1), material).reshape(1, -1), s, tol=lanczos_tol)
    dt_crit = 2.0 / omega_max if omega_max > 0 else math.inf
    return {"omega_max": omega_max, "dt_crit": dt_crit, "dt": gamma * dt_crit, "material": str(material).replace("-", "_"),
            "n_inverted": n_inverted, "lanczos_residual": res}


def device_lowest_modes(op: ModalOperator, points, cells, lmd, mu, k, **kw):
    """:func:`lowest_modes` on the GPU operator, Jacobi-preconditioned with ``diag(K)`` (order 2: ``op.diagonal()``)."""
    import torch

    from .steady import stiffness_diagonal

    if op.order == 2:
        diag = op.diagonal(k=True, m=False)[0]
    else:
        diag = torch.as_tensor(stiffness_diagonal(points, cells, lmd, mu), dtype=torch.float64, device=op.torch_device)
    return lowest_modes(lambda X: op.apply(X)[0], lambda X: op.apply(X, k=False, m=True)[1], k, op.free,
                        diag_k=diag * op.free, **kw)


def modal_report_p2(points, cells10, dirichlet_nodes, E=1e6, nu=0.3, rho=1.0, k=6, device=0) -> dict:
    """What ``drivers modal --order 2`` prints: the order, the sizes, the lowest ``k`` frequencies of the quadratic
    discretisation with their residuals, iteration counts and wall times.  The time-step figures and the critical
    element of :func:`modal_report` belong to the explicit p = 1 solver and are left out."""
    from . import fem_setup as fs

    points = np.ascontiguousarray(points, dtype=np.float64)
    cells10 = np.ascontiguousarray(cells10, dtype=np.int32)
    lmd, mu = fs.lame(E, nu)
    dirichlet = fs.node_to_dof(dirichlet_nodes)
    t0 = time.perf_counter()
    with ModalOperator(points, cells10, dirichlet, lmd, mu, rho, device) as op:
        t1 = _sync(op.torch_device)
        modes = device_lowest_modes(op, points, cells10, lmd, mu, k)
        t2 = _sync(op.torch_device)
    return {"order": 2, "n_nodes": len(points), "n_elems": len(cells10), "n_free_dofs": 3 * len(points) - len(dirichlet),
            "frequencies_hz": modes["frequencies_hz"].tolist(), "residuals": modes["residuals"].tolist(),
            "modes_converged": modes["converged"], "outer_iterations": modes["outer_iterations"],
            "inner_iterations": modes["inner_iterations"],
            "seconds": {"operator_create": t1 - t0, "lowest_modes": t2 - t1}}


def modal_report(points, cells, dirichlet_nodes, E=1e6, nu=0.3, rho=1.0, gamma=0.9, k=6, device=0) -> dict:
    """What ``drivers modal`` prints: sizes, the three time steps, certification, the critical element, the lowest
    ``k`` frequencies with their residuals, iteration counts and wall times."""
    from . import fem_setup as fs

    points = np.ascontiguousarray(points, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    lmd, mu = fs.lame(E, nu)
    dirichlet = fs.node_to_dof(dirichlet_nodes)
    t0 = time.perf_counter()
    op = ModalOperator(points, cells, dirichlet, lmd, mu, rho, device)
    try:
        t1 = _sync(op.torch_device)
        dt = stable_time_step(points, cells, dirichlet_nodes, E, nu, rho, gamma, device, operator=op)
        t2 = _sync(op.torch_device)
        modes = device_lowest_modes(op, points, cells, lmd, mu, k) if k > 0 else None
        t3 = _sync(op.torch_device)
    finally:
        op.close()
    out = {"n_nodes": len(points), "n_elems": len(cells), "n_free_dofs": 3 * len(points) - len(dirichlet),
           **{key: dt[key] for key in ("dt_reference", "dt_crit", "dt_bound", "ratio", "certified", "critical_element",
                                       "n_nonpositive", "omega_max", "omega_bound", "lanczos_residual",
                                       "lanczos_iterations")}}
    if modes is not None:
        out.update({"frequencies_hz": modes["frequencies_hz"].tolist(), "residuals": modes["residuals"].tolist(),
                    "modes_converged": modes["converged"], "outer_iterations": modes["outer_iterations"],
                    "inner_iterations": modes["inner_iterations"]})
    out["seconds"] = {"operator_create": t1 - t0, **dt["seconds"], "time_step_total": t2 - t1, "lowest_modes": t3 - t2}
    return out


def prestressed_modes(op: ModalOperator, u, material, k, tol=1e-8, **kw):
    """The ``k`` lowest pairs of ``K_T(u) x = omega^2 M x`` on the GPU operator: the natural frequencies of the structure
    about the state ``u`` (an ``(n_dof,)`` displacement, NumPy or a float64 CUDA tensor; an equilibrium of ``material``, e.g.
    of :func:`steady.newton_solve_operator`).  Tension stiffens, compression softens, and the lowest ``omega^2`` reaches 0 at
    the buckling load.  ``K_T`` is the block tangent (:meth:`ModalOperator.tangent_apply_block`), ``M`` the handle's consistent
    mass, the Jacobi preconditioner ``diag K`` of the linear operator, as the Newton solve uses it; the iteration is
    :func:`lowest_modes` with ``indefinite=True``, to which ``kw`` goes.

    Returns what :func:`lowest_modes` returns, plus ``stable``, ``lowest_ritz``, ``n_inverted`` (elements neo-Hooke dropped
    from the tangent at ``u``) and ``material``.  At a state that is not a stable equilibrium - a non-positive Rayleigh
    quotient was met - it returns ``stable = False`` with ``lowest_ritz <= 0``, ``converged = False`` and no frequencies
    (``frequencies_hz`` is None), and does not raise."""
    import torch

    mat = _lib.material_id(material)
    if u is None:
        if mat != 0:
            raise ValueError("a nonlinear material needs the state at which its tangent is taken")
    else:
        u = u if torch.is_tensor(u) else torch.as_tensor(np.asarray(u, dtype=np.float64))
        u = (u.to(device=op.torch_device, dtype=torch.float64).reshape(-1) * op.free).contiguous()
    n_inverted = op.tangent_apply_block(u, torch.zeros((1, op.n_dof), dtype=torch.float64, device=op.torch_device), material,
                                        count=True)[1]
    diag = op.diagonal(k=True, m=False)[0]
    out = lowest_modes(lambda X: op.tangent_apply_block(u, X, material), lambda X: op.apply(X, k=False, m=True)[1], k, op.free,
                       diag_k=diag * op.free, tol=tol, indefinite=True, **kw)
    out.update({"n_inverted": int(n_inverted), "material": str(material).replace("-", "_")})
    return out


def prestressed_report(points, cells, dirichlet_nodes, material, load=(0.0, 0.0, 0.0), k=6, load_steps=1, E=1e6, nu=0.3,
                       rho=1.0, device=0, tol=1e-8) -> dict:
    """What ``drivers modal --material svk / neo-hookean`` prints: the natural frequencies of the mesh (either order, by the
    width of ``cells``) about its equilibrium under the body force ``load = (fx, fy, fz)``, next to those of the unloaded
    structure on the same handle.  :func:`steady.newton_solve_operator` to ``u*`` (``tol`` in the true residual, the load in
    ``load_steps`` fractions), :func:`prestressed_modes` at ``u*``, :func:`device_lowest_modes` for the unstressed pair.

    The dict: ``order``, the sizes, ``material``, ``load``; ``newton`` (``converged``, ``residual``, ``newton_iterations``,
    ``cg_iterations``, ``load_steps``, ``n_inverted``, ``tip_deflection`` - the mean of ``-u_y`` over the vertices of ``x = max`` -
    and ``min_det_f``); ``stable``, ``lowest_ritz``, ``frequencies_hz``, ``residuals``, ``modes_converged``;
    ``frequencies_hz_unstressed``; ``omega2_ratio`` (prestressed over unstressed, per mode); the iteration counts of both
    eigen-iterations and ``seconds``.  If Newton does not converge the report says so and holds no modes; at an unstable
    equilibrium it holds ``stable = False``, ``lowest_ritz`` and no prestressed frequencies."""
    import torch

    from . import fem_setup as fs
    from .steady import newton_solve_operator
    from .stress import QuadraticStressRecovery, StressRecovery

    points = np.ascontiguousarray(points, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    if _lib.material_id(material) == 0:
        raise ValueError("prestressed_report is for svk and neo_hookean: a linear operator's modes do not depend on the load")
    lmd, mu = fs.lame(E, nu)
    dirichlet = fs.node_to_dof(dirichlet_nodes)
    n_vert = int(cells[:, :4].max()) + 1 if len(cells) else 0
    tip = np.nonzero(np.abs(points[:n_vert, 0] - points[:, 0].max()) < 1e-9)[0]
    t0 = time.perf_counter()
    with ModalOperator(points, cells, dirichlet, lmd, mu, rho, device) as op:
        t1 = _sync(op.torch_device)
        u, info = newton_solve_operator(op, op.load(load), material, tol=tol, load_steps=load_steps)
        d = torch.as_tensor(np.asarray(u, dtype=np.float64).reshape(-1), device=op.torch_device)
        rec = (QuadraticStressRecovery if op.order == 2 else StressRecovery)(None, None, None, None, operator=op)
        det_f = rec.element(d, energy=False, material=material, measure="cauchy")["det_f"]
        out = {"order": op.order, "n_nodes": op.n_nodes, "n_elems": op.n_elems, "n_free_dofs": int(op.free.sum().item()),
               "material": str(material).replace("-", "_"), "load": [float(c) for c in load],
               "newton": {**{key: info[key] for key in ("converged", "residual", "newton_iterations", "cg_iterations",
                                                         "load_steps", "n_inverted")},
                          "tip_deflection": float(-np.asarray(u).reshape(-1, 3)[tip, 1].mean()),
                          "min_det_f": float(det_f.min())}}
        t2 = _sync(op.torch_device)
        out["seconds"] = {"operator_create": t1 - t0, "newton": t2 - t1}
        if not info["converged"]:
            return out
        modes = prestressed_modes(op, d, material, k)
        t3 = _sync(op.torch_device)
        rest = device_lowest_modes(op, points, cells, lmd, mu, k)
        t4 = _sync(op.torch_device)
    out.update({"stable": modes["stable"], "lowest_ritz": modes["lowest_ritz"], "n_inverted": modes["n_inverted"],
                "frequencies_hz": modes["frequencies_hz"].tolist() if modes["stable"] else None,
                "residuals": modes["residuals"].tolist() if modes["stable"] else None, "modes_converged": modes["converged"],
                "frequencies_hz_unstressed": rest["frequencies_hz"].tolist(), "residuals_unstressed": rest["residuals"].tolist(),
                "omega2_ratio": (modes["omega2"] / rest["omega2"]).tolist() if modes["stable"] else None,
                "outer_iterations": modes["outer_iterations"], "inner_iterations": modes["inner_iterations"],
                "outer_iterations_unstressed": rest["outer_iterations"], "inner_iterations_unstressed": rest["inner_iterations"]})
    out["seconds"].update({"prestressed_modes": t3 - t2, "unstressed_modes": t4 - t3})
    return out
