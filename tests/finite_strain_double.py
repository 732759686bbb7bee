"""NumPy double of the finite-strain element pass of ``csrc/saa_opfs.hip``, written from the definitions and from nothing
else (the reference has no finite-strain code).  Shared by tests/test_finite_strain.py (CPU) and
tests/test_gpu_finite_strain.py.  Lives under tests/: the product never imports it; it is not a test.

In the style of tests/operator_extended.py, whose geometry it reuses (:class:`operator_extended.Extended`: coordinates
centred on the element's first node, adjugate inverses, ``grad N_a`` and the signed ``w_q detJ_q`` at the points of the K
rule - order 1 the one constant gradient with the weight 1/6, order 2 the four Gauss points): ``np.longdouble`` by default,
every contraction an explicit loop over the small index.  With ``H = grad_X u`` (``u`` masked to 0 on Dirichlet dofs) and
``F = I + H`` at every point

* ``svk``: ``E = (H + H^T + H^T H)/2``, ``S = lam tr(E) I + 2 mu E``, ``P = F S``, ``W = lam/2 tr(E)^2 + mu E:E``;
* ``neo_hookean``: ``J = det F``, ``P = mu (F - F^-T) + lam ln(J) F^-T``, ``W = mu/2 (F:F - 3) - mu ln J + lam/2 (ln J)^2``
  with ``F^-T`` the cofactor matrix over ``J`` and ``F:F - 3 = 2 tr(H) + H:H``.  Evaluated as written (``textbook=True``) ``P``
  is an ``O(H)`` difference of ``O(1)`` numbers and ``tr(H) - ln J`` an ``O(H^2)`` difference of ``O(H)`` ones: the relative
  error is ``eps/|H|`` and ``eps/|H|^2``.  The class therefore works from ``H`` and never forms ``F``, in the way
  ``operator_extended.Extended`` avoids its own cancellations: with ``A = cof(H)``,

      J - 1 = tr H + tr A + det H,     ln J = log1p(J - 1),     F^-T - I = (A - H^T - (tr A + det H) I) / J
      P = mu (H - (F^-T - I)) + lam ln J (I + (F^-T - I))
      W = mu/2 ((y - log1p(y)) - (tr cof(e) + det e)) + lam/2 (ln J)^2,   e = 2 E = H + H^T + H^T H,   y = J^2 - 1

  (``cof(I + H) = (1 + tr H) I - H^T + cof(H)``; ``mu/2 (F:F - 3) - mu ln J = mu/2 (tr e - log1p(y))`` and ``y = tr e + tr
  cof(e) + det e``), and ``y - log1p(y)`` is its series ``y^2/2 - y^3/3 + ...`` below ``|y| = 1/4``.  ``W`` goes through ``e``
  and not through ``H:H`` because a rigid rotation leaves ``e`` alone: with ``H = O(1)`` and a strain ``s``, ``mu/2 H:H + mu
  (tr H - ln J)`` is an ``O(s^2)`` difference of ``O(1)`` terms (error ``eps/s^2``), while ``e`` carries ``eps |H|/s``, which is
  what rounding ``u`` once already costs.  The textbook form stays behind the flag only to prove on the CPU that the bar of
  tests/finite_strain_extended.py can fail.  The class runs in ``np.longdouble`` (default), ``np.float64`` (the "stable
  restatement") and ``operator_extended.MP`` (``mpmath.mpf`` objects, which check the longdouble run);

``f_a[i] = sum_q w_q detJ_q sum_k P_q[i][k] dN_a/dX_k(q)`` summed over the elements and set to 0 on Dirichlet dofs, and
separately ``energy_elem[e] = sum_q w_q |detJ_q| W(F_q)`` with the total ``Pi(u)``.  Under ``neo_hookean`` an element with
``!(J > 0)`` at any point is inverted: it contributes 0 to ``f`` and to the energy.  :func:`run` is the float64
central-difference loop with the node update of ``Tools/Dynamic_solver.py:13-20``."""
from __future__ import annotations

import numpy as np

from operator_extended import MP, Extended, conv, log, log1p, scalar, zeros

MATERIALS = ("svk", "neo_hookean")


class FiniteStrain:
    """``f_int(u)``, ``energy_elem(u)`` and ``Pi(u)`` on ``points (n, 3)``, ``cells (ne, 4 or 10)`` in the arithmetic ``T``."""

    def __init__(self, points, cells, lmd, mu, dirichlet_dofs=(), T=np.longdouble, textbook=False):
        self.T, self.textbook = T, bool(textbook)
        self.ext = Extended(points, cells, lmd, mu, 1.0, T)
        self.n_nodes, self.n_elems, self.na, self.nq = self.ext.n_nodes, self.ext.n_elems, self.ext.na, self.ext.nq
        self.cells = self.ext.cells
        self.lmd, self.mu = self.ext.lmd, self.ext.mu
        self.free = np.ones(3 * self.n_nodes, dtype=bool)
        self.free[np.asarray(dirichlet_dofs, dtype=np.int64)] = False

    def gradient(self, u):
        """``H (ne, nq, 3, 3)`` of the masked ``u (3 n,)``."""
        u = np.where(self.free, conv(u, self.T), conv(0.0, self.T))
        return self.ext._grad_u(self.ext._nodes(u[None]))[0]

    def det_f(self, u):
        """``det F (ne, nq)``."""
        return self._cofactors(self._f(self.gradient(u)))[1]

    def _f(self, H):
        F = H.copy()
        for i in range(3):
            F[..., i, i] = F[..., i, i] + 1
        return F

    @staticmethod
    def _cofactors(F):
        C = np.empty_like(F)
        C[..., 0, 0] = F[..., 1, 1] * F[..., 2, 2] - F[..., 1, 2] * F[..., 2, 1]
        C[..., 0, 1] = F[..., 1, 2] * F[..., 2, 0] - F[..., 1, 0] * F[..., 2, 2]
        C[..., 0, 2] = F[..., 1, 0] * F[..., 2, 1] - F[..., 1, 1] * F[..., 2, 0]
        C[..., 1, 0] = F[..., 0, 2] * F[..., 2, 1] - F[..., 0, 1] * F[..., 2, 2]
        C[..., 1, 1] = F[..., 0, 0] * F[..., 2, 2] - F[..., 0, 2] * F[..., 2, 0]
        C[..., 1, 2] = F[..., 0, 1] * F[..., 2, 0] - F[..., 0, 0] * F[..., 2, 1]
        C[..., 2, 0] = F[..., 0, 1] * F[..., 1, 2] - F[..., 0, 2] * F[..., 1, 1]
        C[..., 2, 1] = F[..., 0, 2] * F[..., 1, 0] - F[..., 0, 0] * F[..., 1, 2]
        C[..., 2, 2] = F[..., 0, 0] * F[..., 1, 1] - F[..., 0, 1] * F[..., 1, 0]
        J = F[..., 0, 0] * C[..., 0, 0] + F[..., 0, 1] * C[..., 0, 1] + F[..., 0, 2] * C[..., 0, 2]
        return C, J

    def stress(self, H, material):
        """``(P (ne, nq, 3, 3), W (ne, nq), inverted (ne,) bool)`` at the displacement gradients ``H``."""
        F = self._f(H)
        P, W = zeros(H.shape, self.T), zeros(H.shape[:2], self.T)
        if material == "svk":
            Em = zeros(H.shape, self.T)
            for i in range(3):
                for k in range(3):
                    Em[..., i, k] = H[..., i, k] + H[..., k, i]
                    for l in range(3):
                        Em[..., i, k] = Em[..., i, k] + H[..., l, i] * H[..., l, k]
            Em = Em / 2
            tr = Em[..., 0, 0] + Em[..., 1, 1] + Em[..., 2, 2]
            S = 2 * self.mu * Em
            for i in range(3):
                S[..., i, i] = S[..., i, i] + self.lmd * tr
            for i in range(3):
                for k in range(3):
                    W = W + self.mu * Em[..., i, k] * Em[..., i, k]
                    for l in range(3):
                        P[..., i, k] = P[..., i, k] + F[..., i, l] * S[..., l, k]
            W = W + self.lmd / 2 * tr * tr
            return P, W, np.zeros(self.n_elems, dtype=bool)
        if material != "neo_hookean":
            raise ValueError(f"unknown material {material!r}")
        if self.textbook:
            return self._neo_hookean_textbook(H, F, P, W)
        A, det_h = self._cofactors(H)                                  # cof(H); no entry of F from here on
        tr_h = H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2]
        rest = A[..., 0, 0] + A[..., 1, 1] + A[..., 2, 2] + det_h      # J - 1 - tr H
        x = tr_h + rest
        J = 1 + x
        ok = np.asarray(J > 0, dtype=bool)                             # NaN: not ok
        inverted = ~ok.all(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            xs, Js = np.where(ok, x, conv(0.0, self.T)), np.where(ok, J, conv(1.0, self.T))
            lnJ = log1p(xs, self.T)
            for i in range(3):
                for k in range(3):
                    D = A[..., i, k] - H[..., k, i]                    # (cof F - J I)[i, k]
                    if i == k:
                        D = D - rest
                    G = D / Js                                         # (F^-T - I)[i, k]
                    P[..., i, k] = self.mu * (H[..., i, k] - G) + self.lmd * lnJ * ((1 if i == k else 0) + G)
            # tr E - ln J from e = 2 E = H + H^T + H^T H, which a rotation leaves alone: det(I + e) = J^2 = 1 + y
            e = zeros(H.shape, self.T)
            for i in range(3):
                for k in range(3):
                    e[..., i, k] = H[..., i, k] + H[..., k, i]
                    for l in range(3):
                        e[..., i, k] = e[..., i, k] + H[..., l, i] * H[..., l, k]
            c2, det_e = self._cofactors(e)
            low = c2[..., 0, 0] + c2[..., 1, 1] + c2[..., 2, 2] + det_e  # J^2 - 1 - tr e
            y = e[..., 0, 0] + e[..., 1, 1] + e[..., 2, 2] + low
            ys = np.where(ok & np.asarray(y > -1, dtype=bool), y, conv(0.0, self.T))
            W = self.mu / 2 * (x_minus_log1p(ys, self.T, 2 * lnJ) - low) + self.lmd / 2 * lnJ * lnJ
        return P, W, inverted

    def _neo_hookean_textbook(self, H, F, P, W):
        """The formulas as the definitions give them, from ``F``: what csrc/saa_opfs.hip evaluated at first."""
        C, J = self._cofactors(F)
        ok = np.asarray(J > 0, dtype=bool)
        inverted = ~ok.all(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            Jsafe = np.where(ok, J, conv(1.0, self.T))
            lnJ = log(Jsafe, self.T)
            hh = zeros(H.shape[:2], self.T)
            for i in range(3):
                for k in range(3):
                    FinvT = C[..., i, k] / Jsafe
                    P[..., i, k] = self.mu * (F[..., i, k] - FinvT) + self.lmd * lnJ * FinvT
                    hh = hh + H[..., i, k] * H[..., i, k]
            W = self.mu / 2 * (2 * (H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2]) + hh) - self.mu * lnJ + self.lmd / 2 * lnJ * lnJ
        return P, W, inverted

    def evaluate(self, u, material):
        """``(f (3 n,), energy_elem (ne,), inverted (ne,) bool)``; inverted elements contribute 0 to both."""
        ext = self.ext
        P, W, inverted = self.stress(self.gradient(u), material)
        zero = conv(0.0, self.T)                                       # (selected, not multiplied: a dropped element may hold NaN)
        f = zeros((self.n_elems, self.na, 3), self.T)
        energy = zeros(self.n_elems, self.T)
        for q in range(self.nq):
            energy = energy + np.abs(ext.wdk[:, q]) * W[:, q]
            for i in range(3):
                for k in range(3):
                    f[..., i] = f[..., i] + (ext.wdk[:, q] * P[:, q, i, k])[:, None] * ext.grad[:, q, :, k]
        f = np.where(inverted[:, None, None], zero, f)
        out = ext._scatter(f[None])[0]
        return np.where(self.free, out, zero), np.where(inverted, zero, energy), inverted

    def force(self, u, material):
        return self.evaluate(u, material)[0]

    def total_energy(self, u, material):
        """``Pi(u) = sum_e energy_elem[e]``, summed in element order."""
        e = self.evaluate(u, material)[1]
        total = conv(0.0, self.T)
        for v in e:
            total = total + v
        return total

    def linear_force(self, u):
        """``K u`` of the handle's linear operator (masked on both sides)."""
        u = np.where(self.free, conv(u, self.T), conv(0.0, self.T))
        return np.where(self.free, self.ext.apply_k(u[None])[0], conv(0.0, self.T))


def x_minus_log1p(x, T, log1p_x=None):
    """``x - log1p(x)`` of ``x > -1`` without the cancellation: below ``|x| = 1/4`` the series ``sum_{k >= 2} (-x)^k / k`` by
    Horner's rule, cut where the first dropped term is below the precision of ``T`` times ``x^2/2``; the difference itself
    elsewhere (its relative error there is at most ``8 eps``), with ``log1p_x`` for ``log1p(x)`` where the caller has a better
    one than ``x`` gives (``x = J^2 - 1`` close to -1 knows ``J^2`` only to ``eps / J^2``)."""
    if T is MP:
        import mpmath

        bits = mpmath.mp.prec
    else:
        bits = 53 if np.dtype(T) == np.float64 else 64
    n = bits // 2 + 4                                                  # 2 (1/4)^(n - 1) / (n + 1) < 2^-bits
    p = zeros(x.shape, T) + scalar((-1.0) ** n, T) / n
    for k in range(n - 1, 1, -1):
        p = p * x + scalar((-1.0) ** k, T) / k
    with np.errstate(invalid="ignore", divide="ignore"):
        direct = x - (log1p(x, T) if log1p_x is None else log1p_x)
    return np.where(np.asarray(np.abs(x) < 0.25, dtype=bool), x * x * p, direct)


def run(force, mass, load, live, dt, alpha, ramp, nsteps, d0=None, dn=None, tn=0.0, record=None):
    """``nsteps`` float64 steps of ``Tools/Dynamic_solver.py:13-20`` with the internal force ``force(d0)``:

        d1 = (dt^2 (scale f - f_int) + 2 m d0 - m dn + dt/2 m alpha dn) / (m + alpha m dt / 2),  scale = min(tn, 1) or 1,

    0 where ``live`` is false (Dirichlet dofs, nodes without elements).  Returns ``(d0, dn, tn)``; ``record(step, d1)``."""
    n = len(mass)
    mass, load = np.asarray(mass, dtype=np.float64), np.asarray(load, dtype=np.float64)
    d0 = np.zeros(n) if d0 is None else np.array(d0, dtype=np.float64)
    dn = np.zeros(n) if dn is None else np.array(dn, dtype=np.float64)
    den = mass + alpha * mass * 0.5 * dt
    for i in range(int(nsteps)):
        scale = min(tn, 1.0) if ramp else 1.0
        s = np.asarray(force(d0), dtype=np.float64)
        num = dt * dt * (scale * load - s) + 2.0 * mass * d0 - mass * dn + 0.5 * dt * mass * alpha * dn
        with np.errstate(invalid="ignore", divide="ignore"):
            d1 = np.where(live, num / den, 0.0)
        if record is not None:
            record(i, d1)
        dn, d0 = d0, d1
        tn += dt
    return d0, dn, tn


def smooth_random_field(points, seed, amplitude=1.0):
    """A seeded displacement ``(3 n,)``: a smooth bend-and-twist of the coordinates plus uniform noise of a fifth of it."""
    rng = np.random.default_rng(seed)
    x = np.asarray(points, dtype=np.float64)
    x = x - x.min(axis=0)
    L = x.max()
    a = rng.uniform(0.5, 1.0, size=6) * rng.choice([-1.0, 1.0], size=6)
    u = np.empty_like(x)
    u[:, 0] = a[0] * x[:, 1] * x[:, 0] / L + a[1] * np.sin(2.0 * x[:, 2])
    u[:, 1] = a[2] * (x[:, 0] / L) ** 2 * L + a[3] * x[:, 2] * x[:, 0] / L
    u[:, 2] = a[4] * np.sin(3.0 * x[:, 0] / L) * L / 3 + a[5] * x[:, 1] * x[:, 0] / L
    u = u + 0.2 * np.abs(u).max() * rng.uniform(-1.0, 1.0, size=u.shape)
    return amplitude * u.reshape(-1) / np.abs(u).max()


def scale_to_strain(fs, u, target=0.3, min_det=0.2):
    """``u`` scaled so that ``max|H| = target``, then halved until the double's ``min det F >= min_det``.  Returns the
    float64 field with ``(min det F, max|H|)``."""
    u = np.asarray(u, dtype=np.float64)
    u = u * (target / float(np.abs(fs.gradient(u)).max()))
    for _ in range(20):
        det, hmax = float(fs.det_f(u).min()), float(np.abs(fs.gradient(u)).max())
        if det >= min_det:
            return u, det, hmax
        u = u * 0.75
    raise AssertionError("no scale gives min det F >= %g" % min_det)


def bend(points, tip_rotation, dirichlet_dofs=()):
    """The finite bend of a beam along x clamped at ``x = 0`` into a circular arc in the x-y plane, downwards, with the tip
    rotated by ``tip_rotation`` rad: cross-sections stay plane, normal to the axis and keep their size, so the strain is the
    fibre stretch ``kappa (y - y_mid)`` alone.  0 on Dirichlet dofs: ``(3 n,)`` float64."""
    x = np.asarray(points, dtype=np.float64)
    L = x[:, 0].max()
    kappa = tip_rotation / L
    th = kappa * x[:, 0]
    r = 1.0 / kappa + (x[:, 1] - 0.5 * (x[:, 1].min() + x[:, 1].max()))   # the mid-plane keeps its length
    u = np.zeros_like(x)
    u[:, 0] = r * np.sin(th) - x[:, 0]
    u[:, 1] = r * np.cos(th) - 1.0 / kappa - (r - 1.0 / kappa)
    u = u.reshape(-1)
    u[np.asarray(dirichlet_dofs, dtype=np.int64)] = 0.0
    return u


def rigid_motion(points, angle=0.5, axis=(1.0, 2.0, -1.0), shift=(0.3, -0.2, 0.1)):
    """``u = (R - I) X + c`` with the rotation by ``angle`` rad about ``axis`` (Rodrigues), in longdouble: ``(3 n,)``."""
    T = np.longdouble
    a = np.asarray(axis, dtype=T)
    a = a / np.sqrt((a * a).sum())
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=T)
    K2 = zeros((3, 3), T)
    for i in range(3):
        for k in range(3):
            for l in range(3):
                K2[i, k] = K2[i, k] + Kx[i, l] * Kx[l, k]
    RmI = np.sin(T(angle)) * Kx + (1 - np.cos(T(angle))) * K2
    X = np.asarray(points, dtype=T)
    u = zeros(X.shape, T)
    for i in range(3):
        for k in range(3):
            u[:, i] = u[:, i] + RmI[i, k] * X[:, k]
        u[:, i] = u[:, i] + T(shift[i])
    return u.reshape(-1)


MESHES = ("structured288", "delaunay2", "beam36", "curved288")       # order 1, 1, 2, 2
E, NU, RHO = 1e6, 0.3, 1.0


def mesh(name):
    """``(points, cells, dirichlet_dofs)`` of the four meshes of the finite-strain tests, clamped on the plane ``x = 0``:
    ``structured_beam(2, length=6.0)`` (288 tets = 256 + 32, 117 nodes) and ``delaunay_beam(2)`` at order 1; the 36-tet beam
    (one block) and the curved 288-tet / 625-node fixture of tests/test_gpu_p2_partition.py at order 2."""
    from conftest import load_golden
    from synchronization_avoiding_algorithms_amd.fem_setup import node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import delaunay_beam, plane_nodes, structured_beam, to_quadratic

    if name == "curved288":
        g = load_golden("p2_beam.npz")
        return g["points_curved"].copy(), np.asarray(g["cells10"], dtype=np.int64), np.asarray(g["dirichlet_dofs"], dtype=np.int64)
    if name == "beam36":
        q = to_quadratic(structured_beam(1, length=6.0))
        pts, cells = q.points.copy(), np.asarray(q.tets10, dtype=np.int64)
    else:
        m = structured_beam(2, length=6.0) if name == "structured288" else delaunay_beam(2)
        pts, cells = m.points.copy(), np.asarray(m.tets, dtype=np.int64)
    return pts, cells, np.asarray(node_to_dof(plane_nodes(pts)), dtype=np.int64)


def lame(E, nu):
    return E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu)), E / (2.0 * (1.0 + nu))


def inversion_state(fs, points, background=None):
    """``(node, u (3 n,), elements)``: ``background`` (a gentle field, None: 0, so that the other elements carry a force) plus
    a displacement that moves one vertex ``node`` - and, at order 2, the mid-edge nodes of
    its edges by half as much, so that edges stay straight - through the opposite faces of ALL the elements around it, and
    inverts exactly those under ``neo_hookean`` in the double ``fs`` (``elements``, sorted).  A deterministic search over the
    free vertices, a fixed list of directions and three lengths; the first hit is returned."""
    points = np.asarray(points, dtype=np.float64)
    cells = fs.cells
    dirs = [np.array(d, dtype=np.float64) for d in ((1, 1, 1), (1, -1, 1), (1, 1, -1), (1, -1, -1), (-1, 1, 1), (-1, -1, 1),
                                                     (-1, 1, -1), (-1, -1, -1), (0, 1, 1), (0, -1, 1), (0, 1, -1), (0, -1, -1))]
    for node in np.unique(cells[:, :4]):
        if not fs.free[3 * node:3 * node + 3].all():
            continue
        star = np.nonzero((cells[:, :4] == node).any(axis=1))[0]
        for d in dirs:
            for length in (1.5, 2.5, 4.0):
                u = np.zeros((len(points), 3))
                u[node] = length * d / np.linalg.norm(d)
                base = np.zeros(u.size) if background is None else np.asarray(background, dtype=np.float64)
                if fs.na == 10:
                    from synchronization_avoiding_algorithms_amd.mesh import TET10_EDGES

                    for e in star:
                        for k, (a, b) in enumerate(TET10_EDGES):
                            if node in (cells[e, a], cells[e, b]):
                                u[cells[e, 4 + k]] = 0.5 * u[node]
                inv = fs.evaluate(u.reshape(-1) + base, "neo_hookean")[2]
                if inv.sum() == len(star) and inv[star].all():
                    return int(node), u.reshape(-1) + base, star
    raise AssertionError("no vertex of this mesh inverts exactly its own elements")
