"""NumPy statement of the stress recovery and the stress error estimate of the quadratic (10-node) tetrahedron, on top of
``p2_double.geometry``: the yardstick of ``csrc/saa_stress_p2.hip``, written from the definitions and not from the kernels.

1. Gauss-point stress at the four points of ``Gauss_Legendre(2)``: ``eps_q = sum_a B_a(xi_q) u_a``, ``sigma_q = D eps_q``,
   von Mises, ``W_e = 1/2 sum_q w_q |detJ_q| sigma_q . eps_q``, ``|V_e| = sum_q w_q |detJ_q|``.
2. Element-linear stress ``sigma_h``: the field linear in the barycentric coordinates through the four Gauss values.  Here it
   is found by SOLVING the 4 x 4 system ``sum_v L_v(xi_q) c_v = sigma_q`` by inverting ``L`` numerically (the kernels use the
   closed form ``c_v = sqrt(5) (sigma_q(v) - b S)``); an edge node takes the mean of its two vertices.
3. Recovered nodal stress: the ``|V_e|``-weighted mean of the corner values over a node's elements (``np.add.at``).
4. Error norm with ``C = inv(D)`` as a matrix: nodal form ``sum_p w_p |detJ_p| d_p^T C d_p`` at the fourteen points of
   ``Gauss_Legendre(4)`` with ``d_p = sum_a N_a(xi_p) sigma*_a - sum_v L_v(xi_p) c_v``; element form with the four points.

Lives under tests/: the product never imports it."""
import numpy as np

import p2_double as p2
from stress_double import von_mises
from synchronization_avoiding_algorithms_amd.Tools.Qudrature import Gauss_Legendre
from synchronization_avoiding_algorithms_amd.mesh import TET10_EDGES, structured_beam, to_quadratic


def barycentric(n_quad):
    """``L (nq, 4)`` of the rule's points: ``(1 - xi - eta - zeta, xi, eta, zeta)``."""
    xi, _ = Gauss_Legendre(n_quad)
    xi = np.asarray(xi, dtype=np.float64)
    return np.concatenate([1.0 - xi.sum(axis=1, keepdims=True), xi], axis=1)


def elasticity(lmd, mu):
    D = np.zeros((6, 6))
    D[:3, :3] = lmd
    D[np.arange(3), np.arange(3)] = lmd + 2.0 * mu
    D[np.arange(3, 6), np.arange(3, 6)] = mu
    return D


class NumpyQuadraticStress:
    """The methods of ``stress.QuadraticStressRecovery`` on NumPy arrays."""

    def __init__(self, points, cells10, lmd, mu):
        self.points = np.asarray(points, dtype=np.float64)
        self.cells = np.asarray(cells10, dtype=np.int64)
        self.n_nodes, self.n_elems = len(self.points), len(self.cells)
        self.D = elasticity(lmd, mu)
        self.C = np.linalg.inv(self.D) if mu > 0 and 3 * lmd + 2 * mu > 0 else None
        wd4, self.grad, _ = p2.geometry(self.points, self.cells, 2)           # (ne, 4), (ne, 4, 10, 3)
        self.wd4 = np.abs(wd4)
        w14, self.N14, dN14 = p2.tables(4)                                    # (14,), (14, 10), (14, 10, 3)
        J14 = np.einsum("eai,qaj->eqij", self.points[self.cells], dN14)       # as p2.geometry, without the inverses
        self.wd14 = np.abs(w14[None, :] * np.linalg.det(J14))                 # (ne, 14)
        self.vol = self.wd4.sum(axis=1)
        self.L4, self.L14 = barycentric(2), barycentric(4)                    # (4, 4), (14, 4)

    # ---- definition 1 ------------------------------------------------------------------------------------------------
    def element(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        U = X.reshape(len(X), -1, 3)[:, self.cells]                           # (m, ne, 10, 3)
        H = np.einsum("meai,eqak->meqik", U, self.grad)                       # grad u at the Gauss points
        eps = np.stack([H[..., 0, 0], H[..., 1, 1], H[..., 2, 2], H[..., 1, 2] + H[..., 2, 1], H[..., 0, 2] + H[..., 2, 0],
                        H[..., 0, 1] + H[..., 1, 0]], axis=-1)                # (m, ne, 4, 6)
        sig = eps @ self.D.T
        vm = von_mises(sig)
        W = 0.5 * np.einsum("eq,meqc,meqc->me", self.wd4, sig, eps)
        flat = vm.reshape(len(X), -1)
        return {"sigma": sig, "von_mises": vm, "energy": W, "energy_total": W.sum(axis=1),
                "von_mises_max": flat.max(axis=1), "von_mises_argmax": flat.argmax(axis=1)}

    # ---- definition 2 ------------------------------------------------------------------------------------------------
    def vertex_values(self, sigma):
        """``c (m, ne, 4, 6)``: the linear field through the Gauss values, at the four vertices."""
        S = np.asarray(sigma, dtype=np.float64)
        return np.einsum("vq,meqc->mevc", np.linalg.inv(self.L4), S)          # L4[q, v] c_v = sigma_q

    def corner_values(self, sigma):
        """``(m, ne, 10, 6)``: vertices, then the mean of the two vertices of each edge."""
        c = self.vertex_values(sigma)
        edges = np.stack([0.5 * (c[:, :, a] + c[:, :, b]) for a, b in TET10_EDGES], axis=2)
        return np.concatenate([c, edges], axis=2)

    # ---- definition 3 ------------------------------------------------------------------------------------------------
    def nodal(self, sigma):
        S = np.asarray(sigma, dtype=np.float64)
        vec = S.ndim == 3
        corner = self.corner_values(S[None] if vec else S)
        num = np.zeros((corner.shape[0], self.n_nodes, 6))
        den = np.zeros(self.n_nodes)
        for a in range(10):
            np.add.at(num, (slice(None), self.cells[:, a]), self.vol[None, :, None] * corner[:, :, a])
            np.add.at(den, self.cells[:, a], self.vol)
        out = np.divide(num, den[None, :, None], out=np.zeros_like(num), where=den[None, :, None] > 0)
        return out[0] if vec else out

    # ---- definition 4 ------------------------------------------------------------------------------------------------
    def error(self, sigma, nodal=None, other=None):
        if (nodal is None) == (other is None):
            raise ValueError("exactly one of nodal and other is needed")
        S = np.asarray(sigma, dtype=np.float64)
        vec = S.ndim == 3
        S = S[None] if vec else S
        if nodal is not None:
            N = np.asarray(nodal, dtype=np.float64)
            N = N[None] if N.ndim == 2 else N
            star = np.einsum("pa,meac->mepc", self.N14, N[:, self.cells])     # sigma* at the 14 points
            lin = np.einsum("pv,mevc->mepc", self.L14, self.vertex_values(S))  # sigma_h at the 14 points
            d = star - lin
            eta2 = np.einsum("ep,mepc,mepc->me", self.wd14, d @ self.C, d)
        else:
            O = np.asarray(other, dtype=np.float64)
            d = (O[None] if O.ndim == 3 else O) - S
            eta2 = np.einsum("eq,meqc,cd,meqd->me", self.wd4, d, self.C, d)
        if self.n_elems:
            out = {"eta2": eta2, "eta2_total": eta2.sum(axis=1), "eta2_max": eta2.max(axis=1), "eta2_argmax": eta2.argmax(axis=1)}
        else:
            out = {"eta2": eta2, "eta2_total": np.zeros(len(S)), "eta2_max": np.zeros(len(S)),
                   "eta2_argmax": np.full(len(S), -1)}
        return {k: v[0] for k, v in out.items()} if vec else out

    def estimate(self, X):
        X = np.asarray(X, dtype=np.float64)
        vec = X.ndim == 1
        el = self.element(X.reshape(1, -1) if vec else X)
        out = self.error(el["sigma"], nodal=self.nodal(el["sigma"]))
        out["energy_total"] = el["energy_total"]
        den = 2.0 * el["energy_total"] + out["eta2_total"]
        out["relative"] = np.sqrt(np.divide(out["eta2_total"], den, out=np.zeros_like(den), where=den > 0))
        return {k: v[0] for k, v in out.items()} if vec else out

    def history(self, traj):
        r = self.element(np.asarray(traj).T)
        return {k: r[k] for k in ("energy_total", "von_mises_max", "von_mises_argmax")}

    def gauss_positions(self):
        """Physical positions of the four Gauss points of every element, ``(ne, 4, 3)`` (isoparametric map)."""
        _, N4, _ = p2.tables(2)
        return np.einsum("qa,eai->eqi", N4, self.points[self.cells])

    def close(self):
        pass


def cubic_field(points, D, seed=0, scale=1e-3, cubic=0.3):
    """The quadratic field of ``estimate_double.quadratic_field`` plus the seeded symmetric cubic term
    ``u_i = scale * cubic * T_ijkl x_j x_k x_l / 6`` (T symmetric in j, k, l): the nodal displacement ``(3 n,)`` and a
    function ``stress(x (..., 3)) -> (..., 6)`` of the exact stress, which is quadratic in x."""
    G = np.random.default_rng(seed).normal(size=(3, 3, 3))
    A = G + G.transpose(0, 2, 1)
    R = np.random.default_rng(seed + 1000).normal(size=(3, 3, 3, 3))
    T = sum(R.transpose(0, *p) for p in ((1, 2, 3), (1, 3, 2), (2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1))) / 6.0
    x = np.asarray(points, dtype=np.float64)
    u = 0.5 * scale * np.einsum("nj,ijk,nk->ni", x, A, x) + scale * cubic / 6.0 * np.einsum("ijkl,nj,nk,nl->ni", T, x, x, x)
    Dm = np.asarray(D)

    def stress(y):
        y = np.asarray(y, dtype=np.float64)
        H = scale * np.einsum("ijk,...k->...ij", A, y) + 0.5 * scale * cubic * np.einsum("ijkl,...k,...l->...ij", T, y, y)
        eps = np.stack([H[..., 0, 0], H[..., 1, 1], H[..., 2, 2], H[..., 1, 2] + H[..., 2, 1], H[..., 0, 2] + H[..., 2, 0],
                        H[..., 0, 1] + H[..., 1, 0]], axis=-1)
        return eps @ Dm.T

    return u.reshape(-1), stress


def true_error(ns, sigma, exact_stress):
    """``sqrt(sum_e integral_e (sigma_exact - sigma_h)^T C (sigma_exact - sigma_h))`` of one column's Gauss-point stresses
    ``(ne, 4, 6)`` with the 14-point rule (straight elements)."""
    pos = np.einsum("pa,eai->epi", ns.N14, ns.points[ns.cells])
    lin = np.einsum("pv,evc->epc", ns.L14, ns.vertex_values(sigma[None])[0])
    d = exact_stress(pos) - lin
    return float(np.sqrt(np.einsum("ep,epc,cd,epd->", ns.wd14, d, ns.C, d)))


def cubic_series(make, lmd, mu):
    """``(eta, true error)`` of the cubic field on the 6 x 1 x 1 beam at n = 1, 2, 4 with the recovery ``make(points,
    cells10, u) -> (sigma (ne, 4, 6), eta2_total)``.  Shared by the CPU and the GPU test."""
    etas, errs = [], []
    for n in (1, 2, 4):
        quad = to_quadratic(structured_beam(n, length=6.0))
        ns = NumpyQuadraticStress(quad.points, quad.tets10, lmd, mu)
        u, exact = cubic_field(quad.points, ns.D)
        sigma, eta2 = make(quad.points, quad.tets10, u)
        etas.append(float(np.sqrt(eta2)))
        errs.append(true_error(ns, sigma, exact))
    return etas, errs


def check_cubic_series(etas, errs):
    ratios = [etas[0] / etas[1], etas[1] / etas[2]]
    eff = [a / b for a, b in zip(etas, errs)]
    print("eta", etas, "true error", errs, "eta ratios", ratios, "true ratios", [errs[0] / errs[1], errs[1] / errs[2]],
          "effectivity", eff)
    assert all(3.7 <= r <= 4.3 for r in ratios), ratios
    assert all(0.6 <= e <= 1.0 for e in eff), eff
