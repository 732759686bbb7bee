"""Explicit dynamics on an operator handle of either element order: the time loop of ``Data_prepare.py:215-240`` for one
whole mesh on one GPU, built for the quadratic tetrahedron, for which the reference has none (``Data_prepare.py:43``:
"p=2 only works for steady case, dynamic case requires advanced lumping method").

Two pieces make it work.  The lumped mass is HRZ (:meth:`modal.ModalOperator.lumped_mass`), because the reference's row
sum gives every vertex of a 10-node tetrahedron a negative mass.  The time step is ``gamma * 2/omega_max`` from Lanczos
on the handle (:func:`modal.stable_time_step_operator`), because the reference's edge-length rule
(``Data_prepare.py:147``) lies 1.56 times above the stability limit for this element.  :class:`OperatorStepper` is
the Python face of ``saa_operator_stepper_*``: two launches per step, state on the GPU.  On an order-1 handle it is not a
rival of :class:`solver.HipExplicitSolver` (the LDS-resident step kernel); it serves both orders so that the production
kernel is a second oracle for it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .solver import _dev


class OperatorStepper:
    """``saa_operator_stepper`` on a :class:`modal.ModalOperator` (borrowed: it must stay open while this object lives).
    ``mass`` and ``load`` (the un-ramped ``f``): ``(n_dof,)`` float64, CUDA tensors or arrays, copied.  State
    ``d0 = dn = 0``, ``tn = 0``."""

    def __init__(self, op, mass, load, dt, alpha, ramp=True):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.op = op
        self.n_dof = op.n_dof
        self.dt = float(dt)
        self._traj = None
        m, f = self._vector(mass), self._vector(load)
        _lib.check(self._lib.saa_operator_stepper_create(op._h, _dev(m), _dev(f), float(dt), float(alpha), 1 if ramp else 0,
                                                         C.byref(self._h)))

    def _vector(self, a):
        import torch

        t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float64))
        t = t.to(device=self.op.torch_device, dtype=torch.float64).reshape(-1).contiguous()
        if t.numel() != self.n_dof:
            raise ValueError(f"expected {self.n_dof} values, got {t.numel()}")
        return t

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.saa_operator_stepper_destroy(self._h)
            self._h = C.c_void_p()
        self._traj = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def step(self, n=1):
        _lib.check(self._lib.saa_operator_stepper_step(self._h, int(n)))

    def state(self):
        """``(d0, dn, tn)``: two new ``(n_dof,)`` CUDA tensors and the time, after everything enqueued has finished."""
        import torch

        d0 = torch.empty(self.n_dof, dtype=torch.float64, device=self.op.torch_device)
        dn = torch.empty_like(d0)
        tn = C.c_double()
        _lib.check(self._lib.saa_operator_stepper_get_state(self._h, _dev(d0), _dev(dn), C.byref(tn)))
        return d0, dn, tn.value

    def set_state(self, d0=None, dn=None, tn=0.0):
        """``d0 = d^n``, ``dn = d^(n-1)`` (None: zeros) and the time."""
        a = None if d0 is None else self._vector(d0)
        b = None if dn is None else self._vector(dn)
        _lib.check(self._lib.saa_operator_stepper_set_state(self._h, _dev(a), _dev(b), float(tn)))

    def record(self, n_cols, save_every=1, next_step_index=0, out=None):
        """Switches the recorder on and returns its ``(n_dof, n_cols)`` CUDA matrix (``saa_set_recorder``'s layout and
        meaning: step index ``i`` fills column ``i / save_every`` when ``i % save_every == 0`` and the column exists).
        ``out``: a contiguous float64 CUDA tensor of at least ``n_dof * n_cols`` values to record into instead of a new
        one.  ``n_cols = 0`` switches it off."""
        import torch

        if not n_cols:
            _lib.check(self._lib.saa_operator_stepper_set_recorder(self._h, None, 0, 1, 0))
            self._traj = None
            return None
        if out is None:
            out = torch.zeros((self.n_dof, int(n_cols)), dtype=torch.float64, device=self.op.torch_device)
        elif out.numel() < self.n_dof * int(n_cols):
            raise ValueError(f"the recorder needs {self.n_dof * int(n_cols)} values, got {out.numel()}")
        _lib.check(self._lib.saa_operator_stepper_set_recorder(self._h, _dev(out), int(n_cols), int(save_every),
                                                               int(next_step_index)))
        self._traj = out
        return out.reshape(-1)[: self.n_dof * int(n_cols)].view(self.n_dof, int(n_cols))

    def set_option(self, name: str, value: float):
        """``stored_geometry`` 0 / 1: the order-2 element pass recomputes its Jacobians / reads them from a table."""
        _lib.check(self._lib.saa_operator_stepper_set_option(self._h, name.encode(), float(value)))


def reference_rule_dt(points, cells, E, nu, rho, gamma=0.9) -> float:
    """The reference's edge-length time step (``commons.py:79-90``, ``Data_prepare.py:147``) on the vertex tetrahedra of
    ``cells`` (4 or 10 columns) - for the quadratic element a figure to report, not a step to take."""
    from . import fem_setup as fs

    return float(fs.cfl_dt(np.asarray(points, dtype=np.float64), np.asarray(cells)[:, :4], E, nu, rho, gamma))


def run_dynamics(points, cells, dirichlet_nodes, n_steps, save_every=1, E=1e6, nu=0.3, rho=1.0, fz=0.5, alpha=0.5,
                 gamma=0.9, device=0):
    """What ``drivers dynamics`` computes: the operator of ``cells`` (4 columns: order 1, 10: order 2) clamped on
    ``dirichlet_nodes``, its lumped mass, the reference load ``(0, -fz, -fz)`` ramped over ``t < 1``, ``dt = gamma *
    2/omega_max`` and ``n_steps`` steps recorded every ``save_every``.  Returns ``(trajectory (n_dof, n_cols) array,
    report dict)``."""
    import torch

    from . import fem_setup as fs
    from .modal import ModalOperator, stable_time_step_operator

    points = np.ascontiguousarray(points, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    lmd, mu = fs.lame(E, nu)
    with ModalOperator(points, cells, fs.node_to_dof(dirichlet_nodes), lmd, mu, rho, device) as op:
        mass = op.lumped_mass()
        ts = stable_time_step_operator(op, mass, gamma)
        n_cols = int(n_steps / save_every)
        with OperatorStepper(op, mass, op.load((0.0, -fz, -fz)), ts["dt"], alpha, ramp=True) as st:
            traj = st.record(n_cols, save_every) if n_cols > 0 else None
            st.step(n_steps)
            d0, _, tn = st.state()
            store = traj.cpu().numpy() if traj is not None else np.zeros((op.n_dof, 0))
        d = d0.cpu().numpy().reshape(-1, 3)
        n_vert = int(cells[:, :4].max()) + 1 if len(cells) else 0
        tip = np.nonzero(np.abs(points[:n_vert, 0] - points[:, 0].max()) < 1e-9)[0]
        rule = reference_rule_dt(points, cells, E, nu, rho, gamma)
        report = {"order": op.order, "n_nodes": op.n_nodes, "n_elems": op.n_elems,
                  "n_free_dofs": int(op.free.sum().item()), "dt": ts["dt"], "dt_crit": ts["dt_crit"],
                  "dt_reference_rule": rule, "ratio": rule / ts["dt_crit"], "omega_max": ts["omega_max"], "steps": int(n_steps),
                  "tn": tn, "max_abs_d": float(np.abs(d).max()), "tip_deflection": float(-d[tip, 1].mean())}
    torch.cuda.synchronize(device)
    return store, report
