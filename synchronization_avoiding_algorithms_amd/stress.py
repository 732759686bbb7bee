"""Stress recovery on the GPU: element stress, von Mises, strain energy and volume-weighted nodal averages.

Definitions follow the reference's Voigt conventions (rows xx, yy, zz, yz, xz, xy with engineering shear,
``Mat_construction.py:93-104``; ``D`` of ``commons.py:25-31``):

* ``eps_e = sum_a B_a u_a``, ``sigma_e = D eps_e`` (constant per linear tetrahedron);
* ``vm_e = sqrt(((sxx-syy)^2 + (syy-szz)^2 + (szz-sxx)^2)/2 + 3 (syz^2 + sxz^2 + sxy^2))``;
* ``W_e = |V_e| sigma_e . eps_e / 2`` with ``V_e = detJ/6``; on a consistently oriented mesh ``sum_e W_e = d^T K d / 2``;
* nodal average ``sigma_v = sum_{e at v} |V_e| sigma_e / sum_{e at v} |V_e|`` (0 at a node with no element).

* stress error in the energy norm, ``eta_e^2 = integral_e (sigma_A - sigma_e)^T C (sigma_A - sigma_e) dV`` with ``C = D^-1``:
  against the piecewise-linear field of nodal values (with the nodal average: the Zienkiewicz-Zhu estimate of the
  discretisation error, ``|V_e|/20 (s^T C s + sum_a delta_a^T C delta_a)``, ``delta_a = sigma_A(vertex a) - sigma_e``,
  ``s = sum_a delta_a``) or against a second element field (``|V_e| delta^T C delta``).

The kernels (``saa_operator_stress``, ``saa_operator_nodal_average``, ``saa_operator_stress_error``) run on the
``saa_operator`` handle of
:class:`modal.ModalOperator`, i.e. with the geometry of the K apply.  Its Dirichlet mask is not applied: the displacement
is read as given (recorded trajectories are already 0 on clamped dofs).  Blocks of vectors are ``(m, n)`` tensors, one
column per row, as in :mod:`modal`.  The reference has no counterpart: it stores displacement only.

:class:`QuadraticStressRecovery` is the same for quadratic tetrahedra on an order-2 handle: stress at the four Gauss points
of every element, the recovered nodal stress and the error estimate (``saa_operator_stress_p2``,
``saa_operator_nodal_stress_p2``, ``saa_operator_stress_error_p2``).

Finite strain.  ``element``, ``estimate`` and ``history`` of both classes take ``material="svk"`` or ``"neo_hookean"`` and
``measure="cauchy"`` or ``"pk2"``: the element pass is then ``saa_operator_stress_finite`` (``include/saa_hip.h`` has the
definitions: the second Piola-Kirchhoff stress ``S`` or the Cauchy stress ``sigma`` of the material, its von Mises value,
``det F`` and the stored energy), the layouts are unchanged, and ``nodal`` and ``error`` run the same kernels on the new
fields with the volume weights of the reference configuration.  The default ``material="linear"`` launches exactly what it
always launched.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

VOIGT = ("xx", "yy", "zz", "yz", "xz", "xy")


def von_mises(sigma):
    """Von Mises stress of Voigt stresses ``(..., 6)`` (torch tensor or NumPy array)."""
    s = sigma
    v = 0.5 * ((s[..., 0] - s[..., 1]) ** 2 + (s[..., 1] - s[..., 2]) ** 2 + (s[..., 2] - s[..., 0]) ** 2) \
        + 3.0 * (s[..., 3] ** 2 + s[..., 4] ** 2 + s[..., 5] ** 2)
    return np.sqrt(v) if isinstance(s, np.ndarray) else v.sqrt()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Recovery:
    """What the two recoveries share: the operator and its ownership, the checks of tensors, the column-chunked loops over
    the raw calls, :meth:`estimate` and :meth:`history`.  ``_ROW`` is the shape of an element's stress rows, ``()`` for one
    stress per element and ``(4,)`` for one per Gauss point; the leading dimensions ``6 |row| n_elems`` of ``sigma`` and
    ``|row| n_elems`` of ``von_mises`` follow from it.  A subclass has ``stress_raw`` (keywords ``energy_total``,
    ``von_mises_max``, ``von_mises_argmax``), ``error_raw``, ``nodal``, ``element``, ``error`` and ``_stress_columns``."""

    MAX_COLUMNS = 16
    _ROW = ()

    def _adopt(self, operator, own):
        self._own = own
        self.op = operator
        self._lib = self.op._lib
        self.n_nodes, self.n_elems, self.n_dof = self.op.n_nodes, self.op.n_elems, self.op.n_dof
        self.torch_device = self.op.torch_device

    def close(self):
        if self._own and getattr(self, "op", None) is not None:
            self.op.close()
        self.op = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, t, name):
        import torch

        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
            raise ValueError(f"{name} must be a float64 CUDA tensor")

    def _chunks(self, m):
        """``(first column, columns)`` of the launches that cover ``m`` columns."""
        return [(j, min(self.MAX_COLUMNS, m - j)) for j in range(0, m, self.MAX_COLUMNS)]

    def stress_finite_raw(self, material, measure, m, x, ldx, stress=None, ld_stress=0, von_mises=None, ld_vm=0, det_f=None,
                          ld_det=0, energy=None, ld_elem=0, energy_total=None, von_mises_max=None, von_mises_argmax=None,
                          n_inverted=False):
        """``saa_operator_stress_finite`` with SAA_MATERIAL_* ``material`` and SAA_STRESS_* ``measure`` as integers (any
        value, m and leading dimension: the library checks them).  ``n_inverted=True`` asks for the inverted elements of
        every column, which synchronises the stream, and returns them as a list of ``m`` ints; otherwise None."""
        count = (C.c_int64 * max(int(m), 1))() if n_inverted else None
        _lib.check(self._lib.saa_operator_stress_finite(self.op._h, int(material), int(measure), int(m), _ptr(x), int(ldx),
                                                        _ptr(stress), int(ld_stress), _ptr(von_mises), int(ld_vm),
                                                        _ptr(det_f), int(ld_det), _ptr(energy), int(ld_elem),
                                                        _ptr(energy_total), _ptr(von_mises_max), _ptr(von_mises_argmax),
                                                        count))
        return [int(c) for c in count[:int(m)]] if n_inverted else None

    @staticmethod
    def _finite(material, measure):
        """``None`` for the linear material, otherwise ``(SAA_MATERIAL_*, SAA_STRESS_*, measure name)``."""
        mat = _lib.material_id(material)
        if str(measure) not in _lib.MEASURES:
            raise ValueError(f"unknown measure {measure!r}: one of {', '.join(_lib.MEASURES)}")
        return None if mat == 0 else (mat, _lib.MEASURES[str(measure)], str(measure))

    def _element(self, X, sigma, von_mises, energy, finite=None) -> dict:
        import torch

        self._check(X, "X")
        vec = X.dim() == 1
        X = (X.reshape(1, -1) if vec else X).contiguous()
        if X.shape[1] != self.n_dof:
            raise ValueError(f"expected {self.n_dof} dofs per column, got {X.shape[1]}")
        m, ne, dev = X.shape[0], self.n_elems, self.torch_device
        per = 4 if self._ROW else 1
        out = {}
        if sigma:
            out["sigma"] = torch.empty((m, ne, *self._ROW, 6), dtype=torch.float64, device=dev)
        if von_mises:
            out["von_mises"] = torch.empty((m, ne, *self._ROW), dtype=torch.float64, device=dev)
        if energy:
            out["energy"] = torch.empty((m, ne), dtype=torch.float64, device=dev)
        out["energy_total"] = torch.empty(m, dtype=torch.float64, device=dev)
        out["von_mises_max"] = torch.empty(m, dtype=torch.float64, device=dev)
        out["von_mises_argmax"] = torch.empty(m, dtype=torch.int32, device=dev)
        if finite:
            out["det_f"] = torch.empty((m, ne, *self._ROW), dtype=torch.float64, device=dev)
        inverted = []
        for j, c in self._chunks(m):
            g = {k: v[j] for k, v in out.items()}
            if finite:
                inverted += self.stress_finite_raw(finite[0], finite[1], c, X[j], self.n_dof, g.get("sigma"), 6 * per * ne,
                                                   g.get("von_mises"), per * ne, g["det_f"], per * ne, g.get("energy"), ne,
                                                   g["energy_total"], g["von_mises_max"], g["von_mises_argmax"], n_inverted=True)
            else:
                self._stress_columns(c, X[j], g.get("sigma"), 6 * per * ne, g.get("von_mises"), per * ne, g.get("energy"), ne,
                                     g["energy_total"], g["von_mises_max"], g["von_mises_argmax"])
        out = {k: v[0] for k, v in out.items()} if vec else out
        if finite:
            out["n_inverted"] = inverted[0] if vec else torch.tensor(inverted, dtype=torch.int64)
            out["measure"] = finite[2]
        return out

    def _error(self, S, O, nodal, vec) -> dict:
        """The error of checked, contiguous ``S (m, n_elems, *row, 6)`` against ``O``: ``(m, n_nodes, 6)`` if ``nodal``,
        otherwise shaped like ``S``."""
        import torch

        m, ne, dev = S.shape[0], self.n_elems, self.torch_device
        ld_sigma = 6 * (4 if self._ROW else 1) * ne
        out = {"eta2": torch.empty((m, ne), dtype=torch.float64, device=dev),
               "eta2_total": torch.empty(m, dtype=torch.float64, device=dev),
               "eta2_max": torch.empty(m, dtype=torch.float64, device=dev),
               "eta2_argmax": torch.empty(m, dtype=torch.int32, device=dev)}
        for j, c in self._chunks(m):
            node, oth = (O[j], None) if nodal else (None, O[j])
            self.error_raw(c, S[j], ld_sigma, node, 6 * self.n_nodes, oth, ld_sigma, out["eta2"][j], ne, out["eta2_total"][j:],
                           out["eta2_max"][j:], out["eta2_argmax"][j:])
        return {k: v[0] for k, v in out.items()} if vec else out

    def estimate(self, X, material="linear") -> dict:
        """Zienkiewicz-Zhu estimate of the stress error of displacement columns ``(m, n_dof)`` (or one ``(n_dof,)``
        vector): :meth:`element` stress -> :meth:`nodal` stress -> :meth:`error`.  Returns the dict of :meth:`error` plus
        ``energy_total`` and ``relative = sqrt(eta2_total / (2 energy_total + eta2_total))`` (0 where both vanish).

        With a finite-strain ``material`` the stress is always the second Piola-Kirchhoff stress, over the reference
        configuration: ``eta_e^2 = integral_0 (S* - S_h)^T D^-1 (S* - S_h) dV``.  For ``svk``, ``S = D E`` and this is
        exactly the energy norm of the Green-strain error.  For ``neo_hookean`` ``D`` is only the linearisation of the
        material at the reference configuration, so ``eta`` is a scale in that norm, not an energy of the material.
        ``relative`` keeps its formula with the stored energy in the place of the strain energy; the result gains
        ``n_inverted`` (inverted elements hold ``S_h = 0``)."""
        import torch

        if self._finite(material, "pk2"):
            el = self.element(X, von_mises=False, energy=False, material=material, measure="pk2")
        else:
            el = self.element(X, von_mises=False, energy=False)
        out = self.error(el["sigma"], nodal=self.nodal(el["sigma"]))
        if "n_inverted" in el:
            out["n_inverted"] = el["n_inverted"]
        out["energy_total"] = el["energy_total"]
        den = 2.0 * el["energy_total"] + out["eta2_total"]
        out["relative"] = torch.where(den > 0, out["eta2_total"] / den, torch.zeros_like(den)).sqrt()
        return out

    def history(self, traj, material="linear", measure="cauchy") -> dict:
        """``energy_total``, ``von_mises_max`` and ``von_mises_argmax`` of every column of a row-major
        ``(n_dof, n_cols)`` trajectory (the recorder's and the HDF5 layout), host array or device tensor.  Only the
        reductions are computed; no per-element field is written.  With a finite-strain ``material`` they are those of
        ``measure`` and of the stored energy, and the result gains ``n_inverted`` and ``min_det_f`` per column (``det F`` of
        one launch's columns is written for that, and reduced)."""
        import torch

        finite = self._finite(material, measure)

        if traj.shape[0] != self.n_dof:
            raise ValueError(f"expected {self.n_dof} rows, got {traj.shape[0]}")
        n = traj.shape[1]
        dev = self.torch_device
        out = {"energy_total": torch.empty(n, dtype=torch.float64, device=dev),
               "von_mises_max": torch.empty(n, dtype=torch.float64, device=dev),
               "von_mises_argmax": torch.empty(n, dtype=torch.int32, device=dev)}
        if finite:
            points = (4 if self._ROW else 1) * self.n_elems
            det = torch.empty((min(n, self.MAX_COLUMNS), points), dtype=torch.float64, device=dev)
            out["min_det_f"] = torch.empty(n, dtype=torch.float64, device=dev)
            inverted = []
        for j, c in self._chunks(n):
            if isinstance(traj, torch.Tensor):
                blk = traj[:, j:j + c].to(device=dev, dtype=torch.float64).T.contiguous()
            else:
                blk = torch.from_numpy(np.ascontiguousarray(np.asarray(traj[:, j:j + c], dtype=np.float64).T)).to(dev)
            if finite:
                inverted += self.stress_finite_raw(finite[0], finite[1], c, blk, self.n_dof, det_f=det, ld_det=points,
                                                   energy_total=out["energy_total"][j:], von_mises_max=out["von_mises_max"][j:],
                                                   von_mises_argmax=out["von_mises_argmax"][j:], n_inverted=True)
                if points:
                    out["min_det_f"][j:j + c] = det[:c].amin(dim=1)
                continue
            self.stress_raw(c, blk, self.n_dof, energy_total=out["energy_total"][j:], von_mises_max=out["von_mises_max"][j:],
                            von_mises_argmax=out["von_mises_argmax"][j:])
        if finite:
            out["n_inverted"] = torch.tensor(inverted, dtype=torch.int64)
        return out


class StressRecovery(_Recovery):
    """Stress recovery of one whole mesh on one GPU.  Wraps ``operator`` (a :class:`modal.ModalOperator`, whose mesh
    and material are then used) or builds one with no Dirichlet dofs.  float64 CUDA tensors in and out."""

    MAX_COMPONENTS = 8

    def __init__(self, points, cells, lmd, mu, device=0, operator=None):
        from .modal import ModalOperator

        own = operator is None
        self._adopt(ModalOperator(points, cells, (), lmd, mu, 1.0, device=device) if own else operator, own)

    # ---- raw calls (any m, k and leading dimension: the library checks them) -----------------------------------------
    def stress_raw(self, m, x, ldx, sigma=None, ld_sigma=0, von_mises=None, energy=None, ld_elem=0, energy_total=None,
                   von_mises_max=None, von_mises_argmax=None):
        _lib.check(self._lib.saa_operator_stress(self.op._h, int(m), _ptr(x), int(ldx), _ptr(sigma), int(ld_sigma),
                                                 _ptr(von_mises), _ptr(energy), int(ld_elem), _ptr(energy_total),
                                                 _ptr(von_mises_max), _ptr(von_mises_argmax)))

    def nodal_raw(self, m, k, elem, ld_elem, node, ld_node):
        _lib.check(self._lib.saa_operator_nodal_average(self.op._h, int(m), int(k), _ptr(elem), int(ld_elem), _ptr(node),
                                                        int(ld_node)))

    def error_raw(self, m, sigma_elem, ld_sigma, sigma_node=None, ld_node=0, sigma_other=None, ld_other=0, eta2=None, ld_eta=0,
                  eta2_total=None, eta2_max=None, eta2_argmax=None):
        _lib.check(self._lib.saa_operator_stress_error(self.op._h, int(m), _ptr(sigma_elem), int(ld_sigma), _ptr(sigma_node),
                                                       int(ld_node), _ptr(sigma_other), int(ld_other), _ptr(eta2), int(ld_eta),
                                                       _ptr(eta2_total), _ptr(eta2_max), _ptr(eta2_argmax)))

    def _stress_columns(self, c, x, sigma, ld_sigma, von_mises, ld_vm, energy, ld_elem, *reductions):
        self.stress_raw(c, x, self.n_dof, sigma, ld_sigma, von_mises, energy, ld_elem, *reductions)  # (ld_vm == ld_elem)

    # ---- tensors -------------------------------------------------------------------------------------------------
    def element(self, X, sigma=True, von_mises=True, energy=True, material="linear", measure="cauchy") -> dict:
        """Element fields of a ``(n_dof,)`` vector or an ``(m, n_dof)`` block, in launches of at most 16 columns:
        ``sigma (m, n_elems, 6)``, ``von_mises``, ``energy (m, n_elems)`` (those asked for) and ``energy_total``,
        ``von_mises_max``, ``von_mises_argmax (m,)``.  A vector input drops the leading ``m``.

        ``material="svk"`` or ``"neo_hookean"``: ``sigma`` is the stress of ``measure`` (``"cauchy"`` or ``"pk2"``) at finite
        strain, ``von_mises`` its von Mises value and ``energy`` the stored energy, and the result gains ``det_f (m,
        n_elems)``, ``n_inverted`` (a CPU int64 tensor ``(m,)``, an int for a vector; reading it synchronises) and
        ``measure``.  An inverted element holds 0 in ``sigma``, ``von_mises`` and ``energy``."""
        return self._element(X, sigma, von_mises, energy, self._finite(material, measure))

    def nodal(self, E):
        """Volume-weighted nodal average of element fields ``(m, n_elems, k)`` (or ``(n_elems, k)``) ->
        ``(m, n_nodes, k)``; more than 8 components go in groups of 8."""
        import torch

        self._check(E, "E")
        vec = E.dim() == 2
        E = E.reshape(1, *E.shape) if vec else E
        if E.dim() != 3 or E.shape[1] != self.n_elems:
            raise ValueError(f"expected (m, {self.n_elems}, k) element fields, got {tuple(E.shape)}")
        m, k = E.shape[0], E.shape[2]
        out = torch.empty((m, self.n_nodes, k), dtype=torch.float64, device=self.torch_device)
        for c0 in range(0, k, self.MAX_COMPONENTS):
            kc = min(self.MAX_COMPONENTS, k - c0)
            Ec = E[..., c0:c0 + kc].contiguous()
            Nc = out if kc == k else torch.empty((m, self.n_nodes, kc), dtype=torch.float64, device=self.torch_device)
            for j in range(0, m, self.MAX_COLUMNS):
                c = min(self.MAX_COLUMNS, m - j)
                self.nodal_raw(c, kc, Ec[j], kc * self.n_elems, Nc[j], kc * self.n_nodes)
            if Nc is not out:
                out[..., c0:c0 + kc] = Nc
        return out[0] if vec else out

    def error(self, sigma_elem, nodal=None, other=None) -> dict:
        """Stress error per element in the energy norm: element stresses ``(m, n_elems, 6)`` against exactly one of
        ``nodal (m, n_nodes, 6)`` (interpolated linearly over each element; with :meth:`nodal` of ``sigma_elem`` this is
        the Zienkiewicz-Zhu estimate) and ``other (m, n_elems, 6)`` (a second element field).  Returns ``eta2 (m,
        n_elems)`` and ``eta2_total``, ``eta2_max``, ``eta2_argmax (m,)``, in launches of at most 16 columns.  2-D inputs
        drop the leading ``m``."""
        if (nodal is None) == (other is None):
            raise ValueError("exactly one of nodal and other is needed")
        second, rows, name = (nodal, self.n_nodes, "nodal") if nodal is not None else (other, self.n_elems, "other")
        self._check(sigma_elem, "sigma_elem")
        self._check(second, name)
        vec = sigma_elem.dim() == 2
        S = (sigma_elem.reshape(1, *sigma_elem.shape) if vec else sigma_elem).contiguous()
        O = (second.reshape(1, *second.shape) if second.dim() == 2 else second).contiguous()
        if S.dim() != 3 or tuple(S.shape[1:]) != (self.n_elems, 6):
            raise ValueError(f"expected (m, {self.n_elems}, 6) element stresses, got {tuple(sigma_elem.shape)}")
        if O.dim() != 3 or tuple(O.shape) != (S.shape[0], rows, 6):
            raise ValueError(f"expected {name} of shape ({S.shape[0]}, {rows}, 6), got {tuple(second.shape)}")
        return self._error(S, O, nodal is not None, vec)


class QuadraticStressRecovery(_Recovery):
    """Stress recovery and error estimate of quadratic (10-node) tetrahedra, one whole mesh on one GPU, on an order-2
    handle (``saa_operator_stress_p2``, ``saa_operator_nodal_stress_p2``, ``saa_operator_stress_error_p2``; the
    definitions are in ``include/saa_hip.h``).  Wraps ``operator`` (an order-2 :class:`modal.ModalOperator`, whose mesh and
    material are then used) or builds one with no Dirichlet dofs.  float64 CUDA tensors in and out.

    The element stress lives at the four Gauss points of the K rule: ``sigma (m, n_elems, 4, 6)``.  ``sigma_h`` is the field
    linear in the barycentric coordinates through these four values, the recovered stress ``sigma*`` the quadratic field of
    the ``|V_e|``-weighted nodal means of ``sigma_h``, and ``eta_e^2`` the energy norm of ``sigma* - sigma_h`` over the
    element (14-point rule), or of the difference to a second Gauss-point field (4-point rule)."""

    _ROW = (4,)

    def __init__(self, points, cells10, lmd, mu, device=0, operator=None):
        from .modal import ModalOperator

        own = operator is None
        if own:
            cells10 = np.asarray(cells10)
            if cells10.ndim != 2 or cells10.shape[1] != 10:
                raise ValueError(f"expected (n_elems, 10) cells, got {cells10.shape}")
            operator = ModalOperator(points, cells10, (), lmd, mu, 1.0, device=device)
        elif operator.order != 2:
            raise ValueError("QuadraticStressRecovery needs an order-2 operator; StressRecovery serves order 1")
        self._adopt(operator, own)

    # ---- raw calls (any m and leading dimension: the library checks them) --------------------------------------------
    def stress_raw(self, m, x, ldx, sigma=None, ld_sigma=0, von_mises=None, ld_vm=0, energy=None, ld_elem=0, energy_total=None,
                   von_mises_max=None, von_mises_argmax=None):
        _lib.check(self._lib.saa_operator_stress_p2(self.op._h, int(m), _ptr(x), int(ldx), _ptr(sigma), int(ld_sigma),
                                                    _ptr(von_mises), int(ld_vm), _ptr(energy), int(ld_elem),
                                                    _ptr(energy_total), _ptr(von_mises_max), _ptr(von_mises_argmax)))

    def nodal_raw(self, m, sigma, ld_sigma, sigma_node, ld_node):
        _lib.check(self._lib.saa_operator_nodal_stress_p2(self.op._h, int(m), _ptr(sigma), int(ld_sigma), _ptr(sigma_node),
                                                          int(ld_node)))

    def error_raw(self, m, sigma, ld_sigma, sigma_node=None, ld_node=0, sigma_other=None, ld_other=0, eta2=None, ld_eta=0,
                  eta2_total=None, eta2_max=None, eta2_argmax=None):
        _lib.check(self._lib.saa_operator_stress_error_p2(self.op._h, int(m), _ptr(sigma), int(ld_sigma), _ptr(sigma_node),
                                                          int(ld_node), _ptr(sigma_other), int(ld_other), _ptr(eta2),
                                                          int(ld_eta), _ptr(eta2_total), _ptr(eta2_max), _ptr(eta2_argmax)))

    def _stress_columns(self, c, x, *fields_and_reductions):
        self.stress_raw(c, x, self.n_dof, *fields_and_reductions)

    # ---- tensors -------------------------------------------------------------------------------------------------
    def _gauss(self, S, name):
        """``(m, n_elems, 4, 6)`` contiguous from that or ``(n_elems, 4, 6)``; the second value says which."""
        self._check(S, name)
        vec = S.dim() == 3
        S = (S.reshape(1, *S.shape) if vec else S).contiguous()
        if S.dim() != 4 or tuple(S.shape[1:]) != (self.n_elems, 4, 6):
            raise ValueError(f"expected {name} of shape (m, {self.n_elems}, 4, 6), got {tuple(S.shape)}")
        return S, vec

    def element(self, X, sigma=True, von_mises=True, energy=True, material="linear", measure="cauchy") -> dict:
        """Gauss-point fields of a ``(n_dof,)`` vector or an ``(m, n_dof)`` block, in launches of at most 16 columns:
        ``sigma (m, n_elems, 4, 6)``, ``von_mises (m, n_elems, 4)``, ``energy (m, n_elems)`` (those asked for) and
        ``energy_total``, ``von_mises_max``, ``von_mises_argmax (m,)`` (a point index ``4 e + q``).  A vector input drops
        the leading ``m``.

        ``material="svk"`` or ``"neo_hookean"``: ``sigma`` is the stress of ``measure`` (``"cauchy"`` or ``"pk2"``) at finite
        strain, ``von_mises`` its von Mises value and ``energy`` the stored energy, and the result gains ``det_f (m,
        n_elems, 4)``, ``n_inverted`` (a CPU int64 tensor ``(m,)``, an int for a vector; reading it synchronises) and
        ``measure``.  An inverted element holds 0 in ``sigma``, ``von_mises`` and ``energy``."""
        return self._element(X, sigma, von_mises, energy, self._finite(material, measure))

    def nodal(self, sigma):
        """Recovered nodal stress of Gauss-point stresses ``(m, n_elems, 4, 6)`` (or ``(n_elems, 4, 6)``) ->
        ``(m, n_nodes, 6)``."""
        import torch

        S, vec = self._gauss(sigma, "sigma")
        m = S.shape[0]
        out = torch.empty((m, self.n_nodes, 6), dtype=torch.float64, device=self.torch_device)
        for j in range(0, m, self.MAX_COLUMNS):
            self.nodal_raw(min(self.MAX_COLUMNS, m - j), S[j], 24 * self.n_elems, out[j], 6 * self.n_nodes)
        return out[0] if vec else out

    def error(self, sigma, nodal=None, other=None) -> dict:
        """Stress error per element in the energy norm: Gauss-point stresses ``(m, n_elems, 4, 6)`` against exactly one of
        ``nodal (m, n_nodes, 6)`` (interpolated quadratically; with :meth:`nodal` of ``sigma`` this is the Zienkiewicz-Zhu
        estimate) and ``other (m, n_elems, 4, 6)`` (a second Gauss-point field).  Returns ``eta2 (m, n_elems)`` and
        ``eta2_total``, ``eta2_max``, ``eta2_argmax (m,)``, in launches of at most 16 columns.  Inputs without the leading
        ``m`` drop it."""
        if (nodal is None) == (other is None):
            raise ValueError("exactly one of nodal and other is needed")
        S, vec = self._gauss(sigma, "sigma")
        m, nn = S.shape[0], self.n_nodes
        if nodal is not None:
            self._check(nodal, "nodal")
            O = (nodal.reshape(1, *nodal.shape) if nodal.dim() == 2 else nodal).contiguous()
            if tuple(O.shape) != (m, nn, 6):
                raise ValueError(f"expected nodal of shape ({m}, {nn}, 6), got {tuple(nodal.shape)}")
        else:
            O, _ = self._gauss(other, "other")
            if O.shape[0] != m:
                raise ValueError(f"expected other of {m} columns, got {O.shape[0]}")
        return self._error(S, O, nodal is not None, vec)
