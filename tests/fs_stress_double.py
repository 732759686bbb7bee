"""NumPy double of the finite-strain stress recovery of ``csrc/saa_stress_fs.hip`` (``saa_operator_stress_finite``), written
from the definitions in ``include/saa_hip.h`` on :class:`finite_strain_double.FiniteStrain` (its geometry, its ``H``, its ``W``).
Shared by tests/test_fs_stress.py (CPU) and tests/test_gpu_fs_stress.py.  Lives under tests/: the product never imports it; it
is not a test.

``np.longdouble`` by default (``np.float64`` and ``operator_extended.MP`` run the same statements), every contraction an
explicit loop over the small index.  With ``H = grad_X x`` (``x`` read as given: build the ``FiniteStrain`` WITHOUT Dirichlet
dofs), ``A = cof(H)``:

    J - 1 = tr H + tr A + det H,   det_f = 1 + (J - 1),   ln J = log1p(J - 1),   G = F^-T - I = (A - H^T - (tr A + det H) I) / J

* ``svk``: ``E = (H + H^T + H^T H)/2``, ``S = lam tr(E) I + 2 mu E``, ``sigma = F S F^T / J``;
* ``neo_hookean``: ``S = -mu M + lam ln J (I + M)`` with ``M = G + G^T + G^T G``, ``sigma = (mu (H + H^T + H H^T) + lam ln J I) / J``;
* von Mises of the chosen measure, from differences of the normal stresses that are formed before the common pressure is
  added, so that a pressure ``lambda / mu`` times the deviator costs them nothing: ``2 mu (E_ii - E_jj)`` (``svk``, ``pk2``),
  those of ``(2 mu F E F^T + lam tr(E) (H + H^T + H H^T)) / J`` (``svk``, ``cauchy``: ``F F^T = I + H + H^T + H H^T``, and ``lam
  tr(E) / J`` goes on the diagonal last), ``(lam ln J - mu)(M_ii - M_jj)`` and ``mu (B_ii - B_jj) / J`` with ``B = H + H^T + H
  H^T`` (``neo_hookean``).  ``kernel_order=True`` keeps, for ``svk`` with ``cauchy``, the order this double and the
  kernel had at first: ``F (lam tr(E) I + 2 mu E) F^T / J`` in one piece and the differences of its diagonal;
* ``energy[e] = sum_q w_q |detJ_q| W(F_q)`` with ``W`` of ``FiniteStrain.stress``;
* an element with ``!(J > 0)`` at any point (NaN included) is inverted under ``neo_hookean`` (either measure) and under the
  ``cauchy`` measure (either material): its stress, von Mises and energy are 0, it is left out of the total and the maximum.
  ``svk`` with ``pk2`` does not look at ``J``.  ``det_f`` always holds the computed value.

Voigt rows xx, yy, zz, yz, xz, xy.  Results are ``(ne, nq, ...)`` arrays; the GPU's layouts are their C-order flattening."""
from __future__ import annotations

import numpy as np

from finite_strain_double import FiniteStrain
from operator_extended import MP, conv, log1p, sqrt, zeros

MEASURES = ("pk2", "cauchy")
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def voigt(S):
    """``(..., 3, 3)`` symmetric -> ``(..., 6)``."""
    out = np.empty(S.shape[:-2] + (6,), dtype=S.dtype)
    for c, (i, k) in enumerate(VOIGT):
        out[..., c] = S[..., i, k]
    return out


def tensor(v):
    """``(..., 6)`` Voigt -> ``(..., 3, 3)`` symmetric."""
    out = np.empty(v.shape[:-1] + (3, 3), dtype=v.dtype)
    for c, (i, k) in enumerate(VOIGT):
        out[..., i, k] = v[..., c]
        out[..., k, i] = v[..., c]
    return out


def von_mises(v, d=None, T=None):
    """Von Mises value of Voigt stresses ``(..., 6)``; ``d = (d01, d12, d20)``: the differences of the normal stresses where
    the caller has them from before the common pressure went in (None: taken from ``v``)."""
    if d is None:
        d = v[..., 0] - v[..., 1], v[..., 1] - v[..., 2], v[..., 2] - v[..., 0]
    d01, d12, d20 = d
    return sqrt((d01 * d01 + d12 * d12 + d20 * d20) / 2 + 3 * (v[..., 3] * v[..., 3] + v[..., 4] * v[..., 4] + v[..., 5] * v[..., 5]),
                (MP if v.dtype == object else v.dtype) if T is None else T)


class FsStress:
    """The recovery on ``points (n, 3)``, ``cells (ne, 4 or 10)`` in the arithmetic ``T`` (``np.longdouble``, ``np.float64`` or
    ``operator_extended.MP``); no Dirichlet mask.  ``kernel_order=True``: ``svk`` with ``cauchy`` as ``F (lam tr(E) I + 2
    mu E) F^T / J`` in one piece and its von Mises value from the differences of the finished normal stresses - the order the
    kernel had at first (its other three instantiations took the differences from the strain from the start), kept only to
    prove that the bar of tests/fs_stress_extended.py can fail."""

    def __init__(self, points, cells, lmd, mu, T=np.longdouble, kernel_order=False):
        self.T, self.kernel_order = T, bool(kernel_order)
        self.fs = FiniteStrain(points, cells, lmd, mu, (), T)
        self.n_elems, self.nq = self.fs.n_elems, self.fs.nq
        self.lmd, self.mu = self.fs.lmd, self.fs.mu

    def kinematics(self, H):
        """``(A = cof H, rest = tr A + det H, x = J - 1)`` of ``H (ne, nq, 3, 3)``."""
        A, det_h = self.fs._cofactors(H)
        rest = A[..., 0, 0] + A[..., 1, 1] + A[..., 2, 2] + det_h
        return A, rest, H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2] + rest

    def point_stress(self, H, material, measure, kin=None):
        """``(stress (ne, nq, 3, 3), d, det_f (ne, nq), ok (ne, nq) bool)``: the stress of every point as the formulas give it
        (points with ``!(J > 0)`` hold junk where ``J`` is used), the differences ``d = (d01, d12, d20)`` of its normal
        entries formed before the common pressure is added (``kernel_order`` with ``svk`` and ``cauchy``: after), and ``J > 0``
        where the rule looks at it.  ``kin``: :meth:`kinematics` of ``H`` where the caller has it."""
        T, lmd, mu = self.T, self.lmd, self.mu
        one, zero = conv(1.0, T), conv(0.0, T)
        A, rest, x = self.kinematics(H) if kin is None else kin
        J = 1 + x
        pos = np.asarray(J > 0, dtype=bool)
        ok = np.ones_like(pos) if (material, measure) == ("svk", "pk2") else pos
        Js, xs = np.where(pos, J, one), np.where(pos, x, zero)
        out = zeros(H.shape, T)

        def diffs(D, f=None):
            """The three differences of the diagonal of ``D``, times ``f``."""
            d = D[..., 0, 0] - D[..., 1, 1], D[..., 1, 1] - D[..., 2, 2], D[..., 2, 2] - D[..., 0, 0]
            return d if f is None else tuple(f * v for v in d)

        if material == "svk":
            Em = zeros(H.shape, T)
            for i in range(3):
                for k in range(3):
                    Em[..., i, k] = H[..., i, k] + H[..., k, i]
                    for l in range(3):
                        Em[..., i, k] = Em[..., i, k] + H[..., l, i] * H[..., l, k]
            Em = Em / 2
            S = 2 * mu * Em
            ltr = lmd * (Em[..., 0, 0] + Em[..., 1, 1] + Em[..., 2, 2])
            if measure == "pk2":
                out = S.copy()
                for i in range(3):
                    out[..., i, i] = out[..., i, i] + ltr
                return out, diffs(Em, 2 * mu), J, ok
            F = self.fs._f(H)
            if self.kernel_order:
                for i in range(3):
                    S[..., i, i] = S[..., i, i] + ltr
            for i in range(3):
                for k in range(3):
                    for a in range(3):
                        for b in range(3):
                            out[..., i, k] = out[..., i, k] + F[..., i, a] * S[..., a, b] * F[..., k, b]
            if self.kernel_order:
                out = out / Js[..., None, None]
                return out, diffs(out), J, ok
            # F S F^T = 2 mu F E F^T + lam tr(E) (I + B), B = H + H^T + H H^T: the pressure lam tr(E) / J goes in last
            for i in range(3):
                for k in range(3):
                    B = H[..., i, k] + H[..., k, i]
                    for l in range(3):
                        B = B + H[..., i, l] * H[..., k, l]
                    out[..., i, k] = (out[..., i, k] + ltr * B) / Js
            d = diffs(out)
            for i in range(3):
                out[..., i, i] = out[..., i, i] + ltr / Js
            return out, d, J, ok
        if material != "neo_hookean":
            raise ValueError(f"unknown material {material!r}")
        with np.errstate(invalid="ignore", divide="ignore"):
            lnJ = log1p(xs, T)
        if measure == "pk2":
            G = zeros(H.shape, T)
            for i in range(3):
                for k in range(3):
                    D = A[..., i, k] - H[..., k, i]
                    if i == k:
                        D = D - rest
                    G[..., i, k] = D / Js
            M = zeros(H.shape, T)
            for i in range(3):
                for k in range(3):
                    M[..., i, k] = G[..., i, k] + G[..., k, i]
                    for l in range(3):
                        M[..., i, k] = M[..., i, k] + G[..., l, i] * G[..., l, k]
                    out[..., i, k] = -mu * M[..., i, k] + lmd * lnJ * ((1 if i == k else 0) + M[..., i, k])
            return out, diffs(M, lmd * lnJ - mu), J, ok
        B = zeros(H.shape, T)
        for i in range(3):
            for k in range(3):
                B[..., i, k] = H[..., i, k] + H[..., k, i]
                for l in range(3):
                    B[..., i, k] = B[..., i, k] + H[..., i, l] * H[..., k, l]
                out[..., i, k] = (mu * B[..., i, k] + lmd * lnJ * (1 if i == k else 0)) / Js
        return out, diffs(B, mu / Js), J, ok

    def recover(self, u, material, measure):
        """dict of ``stress (ne, nq, 6)``, ``von_mises (ne, nq)``, ``det_f (ne, nq)``, ``energy (ne,)``, ``inverted (ne,)``
        bool, ``n_inverted``, ``energy_total`` (summed in element order), ``von_mises_max`` and ``von_mises_argmax`` (the
        lowest point index ``nq e + q`` of the maximum; 0.0 and -1 when no point holds a value)."""
        return self.recover_all(u, ((material, measure),))[material, measure]

    def recover_all(self, u, combos=None):
        """``(material, measure) -> recover(u, material, measure)`` for every pair of ``combos`` (None: all four), with ``H``,
        the kinematics and each material's ``W`` formed once."""
        combos = [(a, b) for a in ("svk", "neo_hookean") for b in MEASURES] if combos is None else list(combos)
        for _, measure in combos:
            if measure not in MEASURES:
                raise ValueError(f"unknown measure {measure!r}")
        T, zero = self.T, conv(0.0, self.T)
        H = self.fs.gradient(u)
        kin = self.kinematics(H)
        energies, out = {}, {}
        for material, measure in combos:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                S, d, J, ok = self.point_stress(H, material, measure, kin)
                if material not in energies:
                    W = self.fs.stress(H, material)[1]
                    energy = zeros(self.n_elems, T)
                    for q in range(self.nq):
                        energy = energy + np.abs(self.fs.ext.wdk[:, q]) * W[:, q]
                    energies[material] = energy
                inverted = ~ok.all(axis=1)
                sv = voigt(S)
                vm = von_mises(sv, d, T)
            sv = np.where(inverted[:, None, None], zero, sv)              # (selected, not multiplied: junk may be NaN)
            vm = np.where(inverted[:, None], zero, vm)
            energy = np.where(inverted, zero, energies[material])
            total = zero
            for v in energy:
                total = total + v
            best, arg = conv(-1.0, T), -1
            for p, (v, bad) in enumerate(zip(vm.reshape(-1), np.repeat(inverted, self.nq))):
                if not bad and v > best:
                    best, arg = v, p
            out[material, measure] = {"stress": sv, "von_mises": vm, "det_f": J, "energy": energy, "inverted": inverted,
                                      "n_inverted": int(inverted.sum()), "energy_total": total,
                                      "von_mises_max": best if arg >= 0 else zero, "von_mises_argmax": arg}
        return out

    def linear_stress(self, u):
        """``sigma = lam tr(H) I + mu (H + H^T)`` Voigt ``(ne, nq, 6)``: what the linear entries write."""
        H = self.fs.gradient(u)
        S = zeros(H.shape, self.T)
        tr = H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2]
        for i in range(3):
            for k in range(3):
                S[..., i, k] = self.mu * (H[..., i, k] + H[..., k, i]) + (self.lmd * tr if i == k else 0)
        return voigt(S)

    def first_piola(self, u, material):
        """``P (ne, nq, 3, 3)`` of ``FiniteStrain.stress``."""
        return self.fs.stress(self.fs.gradient(u), material)[0]

    def force_from_pk2(self, u, pk2):
        """``f_int (3 n,)`` rebuilt from PK2 stresses ``(ne, nq, 6)`` (any float type; converted): ``P = F S`` with the double's
        ``F``, gradients and weights, summed over the elements."""
        ext, T = self.fs.ext, self.T
        H = self.fs.gradient(u)
        F = self.fs._f(H)
        S = tensor(conv(pk2, T))
        f = zeros((self.n_elems, self.fs.na, 3), T)
        for q in range(self.nq):
            for i in range(3):
                for k in range(3):
                    P = zeros(self.n_elems, T)
                    for l in range(3):
                        P = P + F[:, q, i, l] * S[:, q, l, k]
                    f[..., i] = f[..., i] + (ext.wdk[:, q] * P)[:, None] * ext.grad[:, q, :, k]
        return ext._scatter(f[None])[0]


def standin(order):
    """The NumPy stand-in recovery of ``drivers.stress_finite`` / ``estimate_finite`` (``recovery=``): the linear double of
    that order (``p2_stress_double.NumpyQuadraticStress``, ``estimate_double.NumpyEstimate``) whose ``element`` and
    ``history`` take ``material=`` and ``measure=`` and then answer with :class:`FsStress` in float64."""
    if order == 2:
        from p2_stress_double import NumpyQuadraticStress as Base
    else:
        from estimate_double import NumpyEstimate as Base
    row = (4,) if order == 2 else ()

    class Standin(Base):
        def __init__(self, points, cells, lmd, mu):
            super().__init__(points, cells, lmd, mu)
            self._fs = FsStress(points, cells, lmd, mu, T=np.float64)

        def element(self, X, material=None, measure="cauchy"):
            if material is None:
                return super().element(X)
            ne, rs = self._fs.n_elems, [self._fs.recover(x, material, measure) for x in np.atleast_2d(X)]
            return {"sigma": np.stack([r["stress"].reshape(ne, *row, 6) for r in rs]),
                    "von_mises": np.stack([r["von_mises"].reshape(ne, *row) for r in rs]),
                    "det_f": np.stack([r["det_f"].reshape(ne, *row) for r in rs]),
                    "energy": np.stack([r["energy"] for r in rs]),
                    "energy_total": np.array([r["energy_total"] for r in rs]),
                    "von_mises_max": np.array([r["von_mises_max"] for r in rs]),
                    "von_mises_argmax": np.array([r["von_mises_argmax"] for r in rs], dtype=np.int32),
                    "n_inverted": np.array([r["n_inverted"] for r in rs], dtype=np.int64), "measure": measure}

        def history(self, traj, material=None, measure="cauchy"):
            if material is None:
                return super().history(traj)
            el = self.element(np.asarray(traj).T, material=material, measure=measure)
            out = {k: el[k] for k in ("energy_total", "von_mises_max", "von_mises_argmax", "n_inverted")}
            out["min_det_f"] = el["det_f"].reshape(len(el["det_f"]), -1).min(axis=1)
            return out

    return Standin
