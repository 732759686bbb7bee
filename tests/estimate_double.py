"""NumPy stand-in of the stress error estimate (the ``recovery`` argument of ``drivers.estimate``) on top of
:class:`stress_double.NumpyStress`, and the quadratic field whose discretisation error is known in closed form.  The
element integral is taken by the 4-point Gauss rule of the tetrahedron (exact for quadratics) with ``C = inv(D)``, so it
shares neither the closed form of the integral nor that of the compliance with the kernel.  Lives under tests/: the
product never imports it."""
import numpy as np

from stress_double import NumpyStress

# 4-point rule, degree 2: barycentric coordinates (a, b, b, b) and permutations, weights |V| / 4
_GA, _GB = (5.0 + 3.0 * np.sqrt(5.0)) / 20.0, (5.0 - np.sqrt(5.0)) / 20.0
GAUSS4 = np.full((4, 4), _GB) + (_GA - _GB) * np.eye(4)          # (point, shape function)


class NumpyEstimate(NumpyStress):
    def __init__(self, points, cells, lmd, mu):
        super().__init__(points, cells, lmd, mu)
        self.C = np.linalg.inv(self.D)

    def error(self, sigma_elem, nodal=None, other=None):
        """``eta2 (m, ne)`` and its total, maximum and (lowest) argmax per column, as ``StressRecovery.error``."""
        if (nodal is None) == (other is None):
            raise ValueError("exactly one of nodal and other is needed")
        S = np.asarray(sigma_elem, dtype=np.float64)
        vec = S.ndim == 2
        S = S[None] if vec else S
        if nodal is not None:
            N = np.asarray(nodal, dtype=np.float64)
            N = N[None] if N.ndim == 2 else N
            corner = N[:, self.cells] - S[:, :, None, :]                # (m, ne, 4, 6): delta_a
            at_q = np.einsum("qa,meac->meqc", GAUSS4, corner)           # the linear field at the Gauss points
            dens = np.einsum("meqc,cd,meqd->me", at_q, self.C, at_q) / 4.0
        else:
            O = np.asarray(other, dtype=np.float64)
            d = (O[None] if O.ndim == 2 else O) - S
            dens = np.einsum("mec,cd,med->me", d, self.C, d)
        eta2 = self.vol * dens
        out = {"eta2": eta2, "eta2_total": eta2.sum(axis=1), "eta2_max": eta2.max(axis=1), "eta2_argmax": eta2.argmax(axis=1)}
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


def quadratic_field(points, D, seed=0, scale=1e-3):
    """``u_i = scale * x^T A_i x / 2`` with ``A_i = G_i + G_i^T``, ``G = default_rng(seed).normal(size=(3, 3, 3))``: the
    nodal displacement ``(3 * n_nodes,)`` and the exact stress at the nodes ``(n_nodes, 6)``, which is linear in x, so
    its nodal interpolant is the exact stress itself."""
    G = np.random.default_rng(seed).normal(size=(3, 3, 3))
    A = G + G.transpose(0, 2, 1)
    x = np.asarray(points, dtype=np.float64)
    u = 0.5 * scale * np.einsum("nj,ijk,nk->ni", x, A, x)
    H = scale * np.einsum("ijk,nk->nij", A, x)                          # H[n, i, j] = d u_i / d x_j
    eps = np.stack([H[:, 0, 0], H[:, 1, 1], H[:, 2, 2], H[:, 1, 2] + H[:, 2, 1], H[:, 0, 2] + H[:, 2, 0],
                    H[:, 0, 1] + H[:, 1, 0]], axis=1)
    return u.reshape(-1), eps @ np.asarray(D).T


def interior_elements(points, cells):
    """Elements with no vertex on a face of the bounding box."""
    x = np.asarray(points, dtype=np.float64)
    on_box = ((x == x.min(axis=0)) | (x == x.max(axis=0))).any(axis=1)
    return ~on_box[np.asarray(cells)].any(axis=1)
