"""NumPy double of the finite-strain stress recovery of ``csrc/saa_stress_fs.hip`` (``saa_operator_stress_finite``), written
from the definitions in ``include/saa_hip.h`` on :class:`finite_strain_double.FiniteStrain` (its geometry, its ``H``, its ``W``).
Shared by tests/test_fs_stress.py (CPU) and tests/test_gpu_fs_stress.py.  Lives under tests/: the product never imports it; it
is not a test.

``np.longdouble`` by default, every contraction an explicit loop over the small index.  With ``H = grad_X x`` (``x`` read as
given: build the ``FiniteStrain`` WITHOUT Dirichlet dofs), ``A = cof(H)``:

    J - 1 = tr H + tr A + det H,   det_f = 1 + (J - 1),   ln J = log1p(J - 1),   G = F^-T - I = (A - H^T - (tr A + det H) I) / J

* ``svk``: ``E = (H + H^T + H^T H)/2``, ``S = lam tr(E) I + 2 mu E``, ``sigma = F S F^T / J``;
* ``neo_hookean``: ``S = -mu M + lam ln J (I + M)`` with ``M = G + G^T + G^T G``, ``sigma = (mu (H + H^T + H H^T) + lam ln J I) / J``;
* von Mises of the chosen measure, ``energy[e] = sum_q w_q |detJ_q| W(F_q)`` with ``W`` of ``FiniteStrain.stress``;
* an element with ``!(J > 0)`` at any point (NaN included) is inverted under ``neo_hookean`` (either measure) and under the
  ``cauchy`` measure (either material): its stress, von Mises and energy are 0, it is left out of the total and the maximum.
  ``svk`` with ``pk2`` does not look at ``J``.  ``det_f`` always holds the computed value.

Voigt rows xx, yy, zz, yz, xz, xy.  Results are ``(ne, nq, ...)`` arrays; the GPU's layouts are their C-order flattening."""
from __future__ import annotations

import numpy as np

from finite_strain_double import FiniteStrain
from operator_extended import conv, log1p, zeros

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


def von_mises(v):
    """Von Mises value of Voigt stresses ``(..., 6)``."""
    d01, d12, d20 = v[..., 0] - v[..., 1], v[..., 1] - v[..., 2], v[..., 2] - v[..., 0]
    return np.sqrt((d01 * d01 + d12 * d12 + d20 * d20) / 2 + 3 * (v[..., 3] * v[..., 3] + v[..., 4] * v[..., 4] + v[..., 5] * v[..., 5]))


class FsStress:
    """The recovery on ``points (n, 3)``, ``cells (ne, 4 or 10)`` in the arithmetic ``T``; no Dirichlet mask."""

    def __init__(self, points, cells, lmd, mu, T=np.longdouble):
        self.T = T
        self.fs = FiniteStrain(points, cells, lmd, mu, (), T)
        self.n_elems, self.nq = self.fs.n_elems, self.fs.nq
        self.lmd, self.mu = self.fs.lmd, self.fs.mu

    def kinematics(self, H):
        """``(A = cof H, rest = tr A + det H, x = J - 1)`` of ``H (ne, nq, 3, 3)``."""
        A, det_h = self.fs._cofactors(H)
        rest = A[..., 0, 0] + A[..., 1, 1] + A[..., 2, 2] + det_h
        return A, rest, H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2] + rest

    def point_stress(self, H, material, measure):
        """``(stress (ne, nq, 3, 3), det_f (ne, nq), ok (ne, nq) bool)``: the stress of every point as the formulas give it
        (points with ``!(J > 0)`` hold junk where ``J`` is used), and ``J > 0`` where the rule looks at it."""
        T, lmd, mu = self.T, self.lmd, self.mu
        one, zero = conv(1.0, T), conv(0.0, T)
        A, rest, x = self.kinematics(H)
        J = 1 + x
        pos = np.asarray(J > 0, dtype=bool)
        ok = np.ones_like(pos) if (material, measure) == ("svk", "pk2") else pos
        Js, xs = np.where(pos, J, one), np.where(pos, x, zero)
        out = zeros(H.shape, T)
        if material == "svk":
            Em = zeros(H.shape, T)
            for i in range(3):
                for k in range(3):
                    Em[..., i, k] = H[..., i, k] + H[..., k, i]
                    for l in range(3):
                        Em[..., i, k] = Em[..., i, k] + H[..., l, i] * H[..., l, k]
            Em = Em / 2
            S = 2 * mu * Em
            tr = Em[..., 0, 0] + Em[..., 1, 1] + Em[..., 2, 2]
            for i in range(3):
                S[..., i, i] = S[..., i, i] + lmd * tr
            if measure == "pk2":
                return S, J, ok
            F = self.fs._f(H)
            for i in range(3):
                for k in range(3):
                    for a in range(3):
                        for b in range(3):
                            out[..., i, k] = out[..., i, k] + F[..., i, a] * S[..., a, b] * F[..., k, b]
            return out / Js[..., None, None], J, ok
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
            for i in range(3):
                for k in range(3):
                    M = G[..., i, k] + G[..., k, i]
                    for l in range(3):
                        M = M + G[..., l, i] * G[..., l, k]
                    out[..., i, k] = -mu * M + lmd * lnJ * ((1 if i == k else 0) + M)
            return out, J, ok
        for i in range(3):
            for k in range(3):
                B = H[..., i, k] + H[..., k, i]
                for l in range(3):
                    B = B + H[..., i, l] * H[..., k, l]
                out[..., i, k] = (mu * B + lmd * lnJ * (1 if i == k else 0)) / Js
        return out, J, ok

    def recover(self, u, material, measure):
        """dict of ``stress (ne, nq, 6)``, ``von_mises (ne, nq)``, ``det_f (ne, nq)``, ``energy (ne,)``, ``inverted (ne,)``
        bool, ``n_inverted``, ``energy_total`` (summed in element order), ``von_mises_max`` and ``von_mises_argmax`` (the
        lowest point index ``nq e + q`` of the maximum; 0.0 and -1 when no point holds a value)."""
        if measure not in MEASURES:
            raise ValueError(f"unknown measure {measure!r}")
        T, zero = self.T, conv(0.0, self.T)
        H = self.fs.gradient(u)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            S, J, ok = self.point_stress(H, material, measure)
            W = self.fs.stress(H, material)[1]
            inverted = ~ok.all(axis=1)
            sv = voigt(S)
            vm = von_mises(sv)
            energy = zeros(self.n_elems, T)
            for q in range(self.nq):
                energy = energy + np.abs(self.fs.ext.wdk[:, q]) * W[:, q]
        sv = np.where(inverted[:, None, None], zero, sv)                  # (selected, not multiplied: junk may be NaN)
        vm = np.where(inverted[:, None], zero, vm)
        energy = np.where(inverted, zero, energy)
        total = zero
        for v in energy:
            total = total + v
        best, arg = conv(-1.0, T), -1
        for p, (v, bad) in enumerate(zip(vm.reshape(-1), np.repeat(inverted, self.nq))):
            if not bad and v > best:
                best, arg = v, p
        return {"stress": sv, "von_mises": vm, "det_f": J, "energy": energy, "inverted": inverted,
                "n_inverted": int(inverted.sum()), "energy_total": total, "von_mises_max": best if arg >= 0 else zero,
                "von_mises_argmax": arg}

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
