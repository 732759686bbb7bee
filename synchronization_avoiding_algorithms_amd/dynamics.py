"""Explicit dynamics on an operator handle of either element order: the time loop of ``Data_prepare.py:215-240`` for one
whole mesh on one GPU, built for the quadratic tetrahedron, for which the reference has none (``Data_prepare.py:43``:
"p=2 only works for steady case, dynamic case requires advanced lumping method").

Two pieces make it work.  The lumped mass is HRZ (:meth:`modal.ModalOperator.lumped_mass`), because the reference's row
sum gives every vertex of a 10-node tetrahedron a negative mass.  The time step is ``gamma * 2/omega_max`` from Lanczos
on the handle (:func:`modal.stable_time_step_operator`), because the reference's edge-length rule
(``Data_prepare.py:147``) lies 1.56 times above the stability limit for this element.  :class:`OperatorStepper` is
the Python face of ``saa_operator_stepper_*``: two launches per step, state on the GPU.  On an order-1 handle it is not a
rival of :class:`solver.HipExplicitSolver` (the LDS-resident step kernel); it serves both orders so that the production
kernel is a second oracle for it.

The partitioned loop the project is named after runs on the same stepper: :class:`OperatorRank` is one rank of a partition
of a replicated mesh of either order (synchronised steps split around a reduction of the shared-node forces, predicted
steps with the shared-dof overwrite), :class:`OperatorPartition` all ranks in one process on one GPU.

``record_energy`` on any of the three switches the energy balance on (``saa_operator_stepper_set_energy``): per step the
kinetic energy ``T`` of the half step, the strain energy in cross form ``U`` and at ``t_n``, the work ``W`` of the load and
the damping loss ``D``.  :func:`energy_balance` turns the rows into ``B_n - B_0``, which stays at round-off over whole-mesh
and synchronised steps and in a predicted window drifts by the energy the predictor injects through the interface.

:class:`ImplicitStepper` is the unconditionally stable integrator on the same handle (``saa_operator_implicit_*``): Newmark's
trapezoidal rule, a Newton iteration per step and a Jacobi-PCG on the shifted tangent, all on the device;
:func:`run_dynamics_newmark` is :func:`run_dynamics` with it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .solver import _dev


class _StepperHandle:
    """What :class:`OperatorStepper` and :class:`ImplicitStepper` share: the handle ``_h`` of a stepper on ``op`` and its life,
    the vectors it takes and the recorder.  A subclass names its two C functions."""

    _destroy = _set_recorder = None             # names of the ``saa_operator_*_destroy`` / ``_set_recorder`` of the subclass

    def _open(self, op, dt):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.op = op
        self.n_dof = op.n_dof
        self.dt = float(dt)
        self._traj = None

    def _vector(self, a):
        import torch

        t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float64))
        t = t.to(device=self.op.torch_device, dtype=torch.float64).reshape(-1).contiguous()
        if t.numel() != self.n_dof:
            raise ValueError(f"expected {self.n_dof} values, got {t.numel()}")
        return t

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
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

    def record(self, n_cols, save_every=1, next_step_index=0, out=None):
        """Switches the recorder on and returns its ``(n_dof, n_cols)`` CUDA matrix (``saa_set_recorder``'s layout and
        meaning: step index ``i`` fills column ``i / save_every`` when ``i % save_every == 0`` and the column exists; the
        implicit stepper records its ``d``).  ``out``: a contiguous float64 CUDA tensor of at least ``n_dof * n_cols`` values
        to record into instead of a new one.  ``n_cols = 0`` switches it off."""
        import torch

        set_recorder = getattr(self._lib, self._set_recorder)
        if not n_cols:
            _lib.check(set_recorder(self._h, None, 0, 1, 0))
            self._traj = None
            return None
        if out is None:
            out = torch.zeros((self.n_dof, int(n_cols)), dtype=torch.float64, device=self.op.torch_device)
        elif out.numel() < self.n_dof * int(n_cols):
            raise ValueError(f"the recorder needs {self.n_dof * int(n_cols)} values, got {out.numel()}")
        _lib.check(set_recorder(self._h, _dev(out), int(n_cols), int(save_every), int(next_step_index)))
        self._traj = out
        return out.reshape(-1)[: self.n_dof * int(n_cols)].view(self.n_dof, int(n_cols))


class OperatorStepper(_StepperHandle):
    """``saa_operator_stepper`` on a :class:`modal.ModalOperator` (borrowed: it must stay open while this object lives).
    ``mass`` and ``load`` (the un-ramped ``f``): ``(n_dof,)`` float64, CUDA tensors or arrays, copied.  State
    ``d0 = dn = 0``, ``tn = 0``.  ``material``: ``linear`` (the default: exactly the kernels of a stepper without a material),
    ``svk`` or ``neo_hookean`` (:meth:`set_material`)."""

    _destroy, _set_recorder = "saa_operator_stepper_destroy", "saa_operator_stepper_set_recorder"

    def __init__(self, op, mass, load, dt, alpha, ramp=True, material="linear"):
        self._open(op, dt)
        self._iface = None
        self._energy = None
        self.n_shared = self.n_global_shared = 0
        m, f = self._vector(mass), self._vector(load)
        _lib.check(self._lib.saa_operator_stepper_create(op._h, _dev(m), _dev(f), float(dt), float(alpha), 1 if ramp else 0,
                                                         C.byref(self._h)))
        self._mass = m                    # (for stable_time_step; the library has its own copy)
        self.steps_done = 0               # (the step count of follow_time_step's records)
        self._anchor = None               # follow_time_step "anchored": (omega_L, Omega(0)), made once
        self.material = "linear"
        if _lib.material_id(material) != 0:
            self.set_material(material)

    def stable_time_step(self, gamma=0.9, lanczos_tol=1e-10):
        """:func:`modal.stable_time_step_operator` with the stepper's mass and material at its current ``d0``: ``omega_max`` of
        ``M_L^-1 K_T(d0)``, ``dt_crit = 2/omega_max`` and what goes with them, plus ``dt`` (the stepper's own, which this call
        does not change) and ``dt_over_dt_crit``: above 1 the linearised update at this state is unstable.  Synchronises."""
        from .modal import stable_time_step_operator

        if _lib.material_id(self.material) == 0:
            out = stable_time_step_operator(self.op, self._mass, gamma, lanczos_tol)
        else:
            out = stable_time_step_operator(self.op, self._mass, gamma, lanczos_tol, self.material, self.state()[0])
        out["dt"] = self.dt
        out["dt_over_dt_crit"] = self.dt / out["dt_crit"]
        return out

    def set_dt(self, dt):
        """An exact change of the step between two steps (``saa_operator_stepper_set_dt``): ``dn`` is replaced so that the
        unchanged step kernels with the new ``dt`` continue the variable-step central-difference scheme; the time, the
        recorder and the inversion counters are left alone.  ``dt`` equal to the current one does nothing.  Enqueued.  Not
        with a shared set, the energy balance or between ``step_begin`` and ``step_finish``."""
        _lib.check(self._lib.saa_operator_stepper_set_dt(self._h, float(dt)))
        self.dt = float(dt)

    def follow_time_step(self, mode, gamma=0.9, grow=1.05, omega_linear=None):
        """One check of the time step at the current state ``d0``: the element bound ``Omega(d0) = max_e omega_e`` of
        :meth:`modal.ModalOperator.tangent_bound` for the stepper's material, a target step from it, and :meth:`set_dt` when
        the target asks for it.  Returns the record ``(step, Omega, target, dt)`` with the steps done and the ``dt`` now in use.

        * ``certified``: ``target = gamma * 2/Omega(d0)``.  ``Omega`` bounds ``omega_max`` of ``M_L^-1 K_T(d0)`` from above (when no
          element has ``detJ <= 0``), so the linearised update at this state is stable - at the price of the bound's pessimism,
          typically a factor 1.4 to 2.3 on well-shaped meshes, more on slivers.
        * ``anchored``: ``target = gamma * (2/omega_L) * min(1, Omega(0)/Omega(d0))`` with ``omega_L`` the Lanczos value of the
          LINEAR operator (``omega_linear``; None: measured once by :func:`modal.stable_time_step_operator`) and ``Omega(0)`` the
          bound at ``u = 0``, computed once.  It follows the stiffening without paying for the pessimism and never exceeds the
          linear operator's step - but it is a HEURISTIC, not a certificate: it assumes that the bound overestimates by the same
          factor at ``d0`` as at 0.

        A target below ``dt`` is taken at once; a target above ``grow * dt`` raises ``dt`` to ``grow * dt``; inside that band nothing
        changes.  RuntimeError if an element's bound is not finite (the state holds NaN or has overflowed).  Synchronises."""
        if mode not in ("certified", "anchored"):
            raise ValueError(f"unknown mode {mode!r}: certified or anchored")
        if not (gamma > 0 and grow >= 1.0):
            raise ValueError("need gamma > 0 and grow >= 1")
        mat = _lib.material_id(self.material)
        bound = self.op.tangent_bound(None if mat == 0 else self.state()[0], self.material)
        if bound["n_nonfinite"] > 0:
            raise RuntimeError(f"follow_time_step: the bound is not finite on {bound['n_nonfinite']} element(s) at step "
                               f"{self.steps_done}: the state holds NaN or has overflowed")
        omega = bound["omega_max"]
        if mode == "certified":
            target = gamma * 2.0 / omega if omega > 0 else float("inf")
        else:
            if self._anchor is None:
                if omega_linear is None:
                    from .modal import stable_time_step_operator

                    omega_linear = stable_time_step_operator(self.op, self._mass, gamma)["omega_max"]
                self._anchor = (float(omega_linear), self.op.tangent_bound(None, "linear")["omega_max"])
            omega_l, omega_0 = self._anchor
            target = gamma * (2.0 / omega_l) * (min(1.0, omega_0 / omega) if omega > 0 else 1.0)
        if target < self.dt:
            self.set_dt(target)
        elif target > grow * self.dt:
            self.set_dt(grow * self.dt)
        return self.steps_done, omega, target, self.dt

    def set_material(self, name):
        """The element pass becomes the finite-strain pass of ``svk`` / ``neo_hookean``, or the linear pass again
        (``saa_operator_stepper_set_material``); clears the inversion counters.  ``dt`` is NOT adapted by the stepper itself: it
        stays what it was, and under large stretch the stability limit moves below the linear operator's
        (:meth:`follow_time_step` adapts it on request)."""
        _lib.check(self._lib.saa_operator_stepper_set_material(self._h, _lib.material_id(name)))
        self.material = str(name).replace("-", "_")

    def inverted(self):
        """``(count, first_step)``: the (element, step) events at which neo-Hooke found an element inverted and dropped its
        contributions since :meth:`set_material` / :meth:`set_state`, and the lowest step index of one (-1: none)."""
        count, first = C.c_int64(0), C.c_int64(-1)
        _lib.check(self._lib.saa_operator_stepper_inverted(self._h, C.byref(count), C.byref(first)))
        return int(count.value), int(first.value)

    def close(self):
        super().close()
        self._energy = None

    def step(self, n=1):
        _lib.check(self._lib.saa_operator_stepper_step(self._h, int(n)))
        self.steps_done += int(n)

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

    def record_energy(self, n_rows, every=1, next_step_index=0, owned=None):
        """Switches the energy balance on and returns its ``(n_rows, 5)`` CUDA matrix of zeros, columns ``T_{n+1/2},
        U_{n+1/2}, U_n, W, D`` (``include/saa_hip.h`` has the definitions and the identity): the step with energy step
        index ``i`` fills row ``i / every`` when ``i % every == 0`` and the row exists; ``W`` and ``D`` run over every step
        from this call on.  ``owned``: one flag per shared node of :meth:`set_shared` - this rank counts the node's mass
        and load terms (None: all).  ``n_rows = 0`` switches it off.  :meth:`set_shared` switches it off too: call this
        after it."""
        import torch

        if not n_rows:
            _lib.check(self._lib.saa_operator_stepper_set_energy(self._h, None, 0, 1, 0, None))
            self._energy = None
            return None
        flags = None
        if owned is not None:
            flags = np.ascontiguousarray(np.asarray(owned).reshape(-1) != 0, dtype=np.uint8)
            if flags.size != self.n_shared:
                raise ValueError(f"owned must hold {self.n_shared} flags, got {flags.size}")
        rows = max(int(n_rows), 0)
        out = torch.zeros((rows, 5), dtype=torch.float64, device=self.op.torch_device)
        _lib.check(self._lib.saa_operator_stepper_set_energy(self._h, _dev(out), int(n_rows), int(every), int(next_step_index),
                                                             flags.ctypes.data if flags is not None and flags.size else None))
        self._energy = out
        return out

    def set_option(self, name: str, value: float):
        """``stored_geometry`` 0 / 1: the order-2 element pass recomputes its Jacobians / reads them from a table."""
        _lib.check(self._lib.saa_operator_stepper_set_option(self._h, name.encode(), float(value)))

    # -- one rank of a partition -----------------------------------------------------------------------------------------
    def set_shared(self, shared_local, shared_slots, n_global_shared):
        """This rank's shared nodes (``RankLayout.shared_local`` / ``shared_slots``) among ``n_global_shared``; a table or
        history row is ``3 * len(shared_local)`` values in that order.  Empty lists and 0 clear the set."""
        a = np.ascontiguousarray(np.asarray(shared_local, dtype=np.int32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(shared_slots, dtype=np.int32).reshape(-1))
        if a.size != b.size:
            raise ValueError("shared_local and shared_slots differ in length")
        ip = C.POINTER(C.c_int32)
        _lib.check(self._lib.saa_operator_stepper_set_shared(self._h, int(a.size), a.ctypes.data_as(ip) if a.size else None,
                                                             b.ctypes.data_as(ip) if b.size else None, int(n_global_shared)))
        self.n_shared, self.n_global_shared = int(a.size), int(n_global_shared)
        self._energy = None

    def set_interface_buffer(self, iface):
        """``iface``: float64 CUDA tensor of ``3 * n_global_shared`` zeros, kept alive here; ``None`` takes it away."""
        if iface is not None and (iface.numel() != 3 * self.n_global_shared or not iface.is_contiguous()):
            raise ValueError("the interface buffer must hold 3 * n_global_shared contiguous doubles")
        _lib.check(self._lib.saa_operator_stepper_set_interface_buffer(self._h, _dev(iface)))
        self._iface = iface

    def _rows(self, t, name, row0, n):
        if t is not None and self.n_shared and (int(row0) < 0 or t.numel() < (int(row0) + int(n)) * 3 * self.n_shared):
            raise ValueError(f"{name} must hold rows {int(row0)} .. {int(row0) + int(n) - 1} of {3 * self.n_shared} values")

    def step_begin(self):
        _lib.check(self._lib.saa_operator_stepper_step_begin(self._h))

    def step_finish(self, hist=None, hist_row=0):
        self._rows(hist, "hist", hist_row, 1)
        _lib.check(self._lib.saa_operator_stepper_step_finish(self._h, _dev(hist), int(hist_row)))
        self.steps_done += 1

    def step_predicted(self, n, table, table_row0=0, hist=None, hist_row0=0):
        self._rows(table, "table", table_row0, n)
        self._rows(hist, "hist", hist_row0, n)
        _lib.check(self._lib.saa_operator_stepper_step_predicted(self._h, int(n), _dev(table), int(table_row0), _dev(hist),
                                                                 int(hist_row0)))
        self.steps_done += int(n)

    def halo_gather(self, row):
        self._rows(row, "row", 0, 1)
        _lib.check(self._lib.saa_operator_stepper_halo_gather(self._h, _dev(row)))

    def halo_scatter(self, row):
        self._rows(row, "row", 0, 1)
        _lib.check(self._lib.saa_operator_stepper_halo_scatter(self._h, _dev(row)))


class ImplicitStepper(_StepperHandle):
    """``saa_operator_implicit`` on a :class:`modal.ModalOperator` (borrowed: it must stay open while this object lives, and it
    serves one stepper at a time).  Newmark with ``beta = 1/4``, ``gamma = 1/2`` (the trapezoidal rule) on the system
    :class:`OperatorStepper` integrates explicitly - ``m a + alpha m v + f_int(d) = scale(t) f`` - so ``dt`` is chosen by the
    physics, not by the stiffest element.  Per step a Newton iteration whose systems ``(K_T(x) + (4/dt^2 + 2 alpha/dt) m) dx = r``
    are solved by a Jacobi-PCG that runs on the device (``include/saa_hip.h`` states the scheme, the convergence rule and what
    is not provided: no line search, no automatic cut of ``dt``, no HHT-alpha, no consistent mass, no partitions, no energy
    table).  ``mass`` and ``load`` (the un-ramped ``f``): ``(n_dof,)`` float64, CUDA tensors or arrays, copied.  State ``d = v =
    0``, ``t = 0`` and the acceleration of the balance there (:meth:`set_state`)."""

    REASONS = {0: "ok", 1: "max_newton", 2: "non_finite", 3: "inverted"}

    _destroy, _set_recorder = "saa_operator_implicit_destroy", "saa_operator_implicit_set_recorder"

    def __init__(self, op, mass, load, dt, alpha, ramp=True, material="linear"):
        self._open(op, dt)
        self.material = str(material).replace("-", "_")
        m, f = self._vector(mass), self._vector(load)
        _lib.check(self._lib.saa_operator_implicit_create(op._h, _dev(m), _dev(f), float(dt), float(alpha), 1 if ramp else 0,
                                                          _lib.material_id(material), C.byref(self._h)))
        self.steps_done = 0

    def step(self, n=1):
        """Up to ``n`` steps.  Returns ``steps_done``, ``converged``, ``reason`` (0 ok, 1 ``max_newton`` reached, 2 a residual
        not finite, 3 an inverted element under neo-Hooke) with its name in ``reason_name``, ``newton_iterations``,
        ``cg_iterations`` (totals of the call) and ``residual`` (the last relative one).  A step that is not accepted leaves the
        state, the time and the step index those of the last accepted step, bit for bit; it does not raise."""
        info = _lib.ImplicitInfo()
        _lib.check(self._lib.saa_operator_implicit_step(self._h, int(n), C.byref(info)))
        self.steps_done += int(info.steps_done)
        return {"steps_done": int(info.steps_done), "converged": bool(info.converged), "reason": int(info.reason),
                "reason_name": self.REASONS.get(int(info.reason), "?"), "newton_iterations": int(info.newton_iterations),
                "cg_iterations": int(info.cg_iterations), "residual": float(info.residual)}

    def state(self):
        """``(d, v, a, t)``: three new ``(n_dof,)`` CUDA tensors and the time, after everything enqueued has finished."""
        import torch

        d = torch.empty(self.n_dof, dtype=torch.float64, device=self.op.torch_device)
        v, a = torch.empty_like(d), torch.empty_like(d)
        t = C.c_double()
        _lib.check(self._lib.saa_operator_implicit_get_state(self._h, _dev(d), _dev(v), _dev(a), C.byref(t)))
        return d, v, a, t.value

    def set_state(self, d=None, v=None, t=0.0):
        """Displacement and velocity (None: zeros; masked on Dirichlet dofs and at nodes without elements) and the time; the
        acceleration is that of the balance at this state, ``(scale(t) f - f_int(d) - alpha m v) / m``."""
        a = None if d is None else self._vector(d)
        b = None if v is None else self._vector(v)
        _lib.check(self._lib.saa_operator_implicit_set_state(self._h, _dev(a), _dev(b), float(t)))

    def set_dt(self, dt):
        """A new step from the next step on: the scheme is one-step, only the shift and the preconditioner are recomputed."""
        _lib.check(self._lib.saa_operator_implicit_set_dt(self._h, float(dt)))
        self.dt = float(dt)

    def set_option(self, name: str, value: float):
        """``tol`` (1e-10), ``max_newton`` (25), ``max_cg`` (20 n_dof per solve), ``check_every`` (25: PCG iterations between
        two looks of the host at the status block)."""
        _lib.check(self._lib.saa_operator_implicit_set_option(self._h, name.encode(), float(value)))


def energy_balance(rows):
    """``B_n - B_0`` of ``(n, 5)`` energy rows ``T, U_{n+1/2}, U_n, W, D``, ``B = T + U_{n+1/2} - W + D``: round-off over
    whole-mesh and synchronised steps; in a predicted window the energy injected through the interface.  NumPy array or
    tensor in, the same out."""
    b = rows[:, 0] + rows[:, 1] - rows[:, 3] + rows[:, 4]
    return b - b[0] if len(b) else b


def shared_ownership(layouts, n_global_shared):
    """Per rank, one flag per entry of its ``shared_local``: the rank is the lowest holder of that shared node."""
    owner = np.full(int(n_global_shared), len(layouts), dtype=np.int64)
    for lay in layouts:
        slots = np.asarray(lay.shared_slots, dtype=np.int64)
        owner[slots] = np.minimum(owner[slots], int(lay.rank))
    return [owner[np.asarray(lay.shared_slots, dtype=np.int64)] == int(lay.rank) for lay in layouts]


class OperatorRank:
    """One rank of a partition of a replicated mesh of either order (``Data_prepare.py:104-209`` for one rank): its
    :class:`fem_setup.RankLayout` (from ``build_layouts`` on the 4- or 10-column cells), a :class:`modal.ModalOperator` on
    its own elements, an :class:`OperatorStepper` with the rank's shared set, and its interface buffer ``iface``.

    ``mass`` and ``load`` are the GLOBAL ``(3 n,)`` vectors; they are restricted with ``layout.local_dof`` as the reference
    does (``Data_prepare.py:175-202``), so a shared node carries the other ranks' contributions too.  ``reduce(iface)``
    sums the interface buffer over the ranks in place between the two halves of a synchronised step:
    ``torch.distributed.all_reduce`` makes this a rank of a multi-process run; ``None`` is a world of one.  The object
    presents what :func:`distributed.run_hybrid` uses.

    ``layouts`` (all ranks', as ``build_layouts`` returns them) settles which shared nodes this rank owns for the energy
    balance: those of which it is the lowest holder.  Without it :meth:`record_energy` counts every shared node as owned,
    which is right for a world of one only."""

    def __init__(self, points, layout, global_shared, mass, load, lmd, mu, rho, dt, alpha, reduce=None, ramp=True, device=0,
                 stored_geometry=None, layouts=None, material="linear"):
        import torch

        from .modal import ModalOperator

        self.layout, self.rank, self.reduce = layout, int(layout.rank), reduce
        self.n_global_shared = len(global_shared)
        points = np.asarray(points, dtype=np.float64)
        self.op = ModalOperator(points[layout.nodes], layout.cells_local, layout.dirichlet_dofs, lmd, mu, rho, device)
        self.tensor_device = self.op.torch_device
        dof = torch.as_tensor(np.asarray(layout.local_dof, dtype=np.int64), device=self.tensor_device)

        def local(a):
            t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.float64))
            return t.to(device=self.tensor_device, dtype=torch.float64).reshape(-1)[dof]

        self.global_dof = dof
        self.stepper = OperatorStepper(self.op, local(mass), local(load), dt, alpha, ramp=ramp, material=material)
        if stored_geometry is not None:
            self.stepper.set_option("stored_geometry", stored_geometry)
        self.stepper.set_shared(layout.shared_local, layout.shared_slots, self.n_global_shared)
        self.iface = torch.zeros(3 * self.n_global_shared, dtype=torch.float64, device=self.tensor_device)
        self.stepper.set_interface_buffer(self.iface)
        self.input_size = 3 * len(layout.shared_local)              # Online_predictor.py:126
        self.owned = None if layouts is None else shared_ownership(layouts, self.n_global_shared)[
            [int(lay.rank) for lay in layouts].index(self.rank)]
        self.dt = float(dt)
        self.steps_done = 0

    def step_synced(self, nsteps=1, hist=None, hist_row0=0):
        """``MODEL=False`` steps: node pass, ``reduce(iface)``, shared-node update; ``hist`` row ``hist_row0 + k``."""
        for k in range(int(nsteps)):
            self.stepper.step_begin()
            if self.reduce is not None:
                self.reduce(self.iface)
            self.stepper.step_finish(hist, hist_row0 + k)
        self.steps_done += int(nsteps)

    def step_local(self, nsteps=1):
        """``MODEL=True`` steps without overwrite: the rank advances on its own partial forces."""
        self.stepper.step(nsteps)
        self.steps_done += int(nsteps)

    def step_predicted(self, nsteps, table, table_row0=0, hist=None, hist_row0=0):
        self.stepper.step_predicted(nsteps, table, table_row0, hist, hist_row0)
        self.steps_done += int(nsteps)

    def get_state(self):
        return self.stepper.state()

    def record_energy(self, n_rows, every=1, next_step_index=0):
        """This rank's share of the energy rows (:meth:`OperatorStepper.record_energy` with the rank's ownership flags):
        the shares of all ranks add up to the rows of the whole mesh."""
        return self.stepper.record_energy(n_rows, every, next_step_index, self.owned)

    def close(self):
        self.stepper.close()
        self.op.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sum_interfaces(ranks, total):
    """The reduction of a one-process partition: the ranks' interface buffers summed in rank order into ``total``, which is
    copied back to every rank."""
    total.copy_(ranks[0].iface)
    for r in ranks[1:]:
        total += r.iface
    for r in ranks:
        r.iface.copy_(total)


class OperatorPartition:
    """All ``P`` ranks of a partition in one process on one GPU: the one-GPU rehearsal of the partitioned loop.  The
    whole-mesh operator is built once for the lumped mass (HRZ for order 2), the load ``(0, -fz, -fz)`` and ``dt = gamma *
    2/omega_max`` (``dt`` given: taken as is; ``lame = (lambda, mu)`` given: instead of ``E``, ``nu``); then one
    :class:`OperatorRank` per part of ``epart``.  ``material``: every rank's (``dt`` stays the linear operator's)."""

    def __init__(self, points, cells, dirichlet_nodes, epart, n_parts=None, E=1e6, nu=0.3, rho=1.0, fz=0.5, alpha=0.5, gamma=0.9,
                 ramp=True, device=0, stored_geometry=None, dt=None, lame=None, material="linear"):
        import torch

        from . import fem_setup as fs
        from .modal import ModalOperator, stable_time_step_operator

        points = np.ascontiguousarray(points, dtype=np.float64)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        epart = np.asarray(epart)
        self.n_parts = int(n_parts) if n_parts is not None else int(epart.max()) + 1
        self.n_dof = 3 * len(points)
        dirichlet_nodes = np.asarray(dirichlet_nodes, dtype=np.int64)
        lmd, mu = lame if lame is not None else fs.lame(E, nu)
        with ModalOperator(points, cells, fs.node_to_dof(dirichlet_nodes), lmd, mu, rho, device) as op:
            self.order, self.tensor_device = op.order, op.torch_device
            mass, load = op.lumped_mass(), op.load((0.0, -fz, -fz))
            self.time_step = {"dt": float(dt)} if dt is not None else stable_time_step_operator(op, mass, gamma)
            torch.cuda.synchronize(device)
        self.dt = self.time_step["dt"]
        layouts, self.global_shared = fs.build_layouts(cells, epart, self.n_parts, len(points), dirichlet_nodes)
        self.ranks = [OperatorRank(points, lay, self.global_shared, mass, load, lmd, mu, rho, self.dt, alpha, None, ramp, device,
                                   stored_geometry, layouts, material) for lay in layouts]
        self.material = str(material).replace("-", "_")
        self._energy = None
        self._sum = torch.zeros(3 * len(self.global_shared), dtype=torch.float64, device=self.tensor_device)

    def reduce_in_rank_order(self):
        sum_interfaces(self.ranks, self._sum)

    def step_synced(self, n=1, hists=None, row0=0):
        """``n`` synchronised steps of every rank in lockstep: all ``begin``, the sum, all ``finish``.  ``hists``: one
        history tensor per rank (or None), row ``row0 + k`` written by step ``k``."""
        for k in range(int(n)):
            for r in self.ranks:
                r.stepper.step_begin()
            self.reduce_in_rank_order()
            for i, r in enumerate(self.ranks):
                r.stepper.step_finish(None if hists is None else hists[i], row0 + k)
        for r in self.ranks:
            r.steps_done += int(n)

    def step_predicted(self, n, tables, table_row0=0, hists=None, hist_row0=0):
        for i, r in enumerate(self.ranks):
            r.step_predicted(n, tables[i], table_row0, None if hists is None else hists[i], hist_row0)

    def run_hybrid(self, n_steps, predictors, n_past, n_future, filter_size):
        """The schedule of :func:`distributed.run_hybrid` without resync, all ranks in lockstep: ``n_past * filter_size``
        synchronised steps, then windows of ``n_future * filter_size`` predicted steps from ``predictors[r](i, hist_r)``.
        Returns the per-rank ``(n_steps, input_size)`` histories."""
        import torch

        hists = [torch.zeros((int(n_steps), r.input_size), dtype=torch.float64, device=self.tensor_device) for r in self.ranks]
        warm, window = int(n_past) * int(filter_size), int(n_future) * int(filter_size)
        i = min(warm, int(n_steps))
        self.step_synced(i, hists, 0)
        while i < n_steps:
            tables = [predictors[k](i, hists[k]) for k in range(self.n_parts)]
            todo = min(window, int(n_steps) - i)
            self.step_predicted(todo, tables, 0, hists, i)
            i += todo
        return hists

    def record_energy(self, n_rows, every=1, next_step_index=0):
        """Switches the energy balance on on every rank; returns the per-rank ``(n_rows, 5)`` tensors (each rank's share)."""
        self._energy = [r.record_energy(n_rows, every, next_step_index) for r in self.ranks]
        if not n_rows:
            self._energy = None
        return self._energy

    def energy(self):
        """The sum of the ranks' energy rows in rank order, a new ``(n_rows, 5)`` tensor: the rows of the whole mesh."""
        if self._energy is None:
            raise RuntimeError("record_energy has not been called")
        total = self._energy[0].clone()
        for e in self._energy[1:]:
            total += e
        return total

    def inverted(self):
        """``(count, first_step)`` of :meth:`OperatorStepper.inverted` over the ranks: the counts summed (an element lives on
        one rank), the lowest first step (-1: none)."""
        each = [r.stepper.inverted() for r in self.ranks]
        firsts = [f for _, f in each if f >= 0]
        return sum(c for c, _ in each), (min(firsts) if firsts else -1)

    def gather(self, which="d0"):
        """The global ``(3 n,)`` CUDA vector of ``d0`` or ``dn``; a shared node comes from its lowest holder."""
        import torch

        if which not in ("d0", "dn"):
            raise ValueError("which must be d0 or dn")
        out = torch.zeros(self.n_dof, dtype=torch.float64, device=self.tensor_device)
        for r in reversed(self.ranks):
            out[r.global_dof] = r.get_state()[0 if which == "d0" else 1]
        return out

    @property
    def tn(self):
        return self.ranks[0].get_state()[2]

    def close(self):
        for r in self.ranks:
            r.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def reference_rule_dt(points, cells, E, nu, rho, gamma=0.9) -> float:
    """The reference's edge-length time step (``commons.py:79-90``, ``Data_prepare.py:147``) on the vertex tetrahedra of
    ``cells`` (4 or 10 columns) - for the quadratic element a figure to report, not a step to take."""
    from . import fem_setup as fs

    return float(fs.cfl_dt(np.asarray(points, dtype=np.float64), np.asarray(cells)[:, :4], E, nu, rho, gamma))


def energy_report(rows):
    """What ``drivers dynamics --energy`` prints of ``(n, 5)`` energy rows (NumPy): the last ``T, U (cross form), W, D``,
    the largest ``|B_n - B_0|`` and the scale it is relative to, ``max_n(W_n, (T + U)_n)``."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    if not len(rows):
        return {"rows": 0}
    last = rows[-1]
    return {"rows": len(rows), "T": float(last[0]), "U": float(last[1]), "W": float(last[3]), "D": float(last[4]),
            "max_abs_balance": float(np.abs(energy_balance(rows)).max()),
            "scale": float(max(rows[:, 3].max(), (rows[:, 0] + rows[:, 1]).max()))}


def run_dynamics(points, cells, dirichlet_nodes, n_steps, save_every=1, E=1e6, nu=0.3, rho=1.0, fz=0.5, alpha=0.5,
                 gamma=0.9, device=0, epart=None, energy_every=0, material="linear", dt_check_every=0, dt_follow=None,
                 dt_follow_every=10):
    """What ``drivers dynamics`` computes: the operator of ``cells`` (4 columns: order 1, 10: order 2) clamped on
    ``dirichlet_nodes``, its lumped mass, the reference load ``(0, -fz, -fz)`` ramped over ``t < 1``, ``dt = gamma *
    2/omega_max`` and ``n_steps`` steps recorded every ``save_every``.  Returns ``(trajectory (n_dof, n_cols) array,
    report dict)``.  ``epart`` (element -> part): the same run through :class:`OperatorPartition`, every rank recording
    its own nodes; the report gains ``parts``, ``n_global_shared`` and ``shared_per_rank``.  ``energy_every = S > 0``: the
    energy balance is recorded every ``S`` steps, the report gains ``energy`` (:func:`energy_report`) and the return value
    a third member, the ``(ceil(n_steps / S), 5)`` table (of a partition: the sum of the ranks' shares).  ``material``:
    ``linear``, ``svk`` or ``neo_hookean``; with a nonlinear one the report gains ``material``, ``inverted`` and
    ``first_inverted_step`` (with ``linear`` it is what it always was, key for key).  ``dt``
    stays that of the linear operator at the reference configuration whatever the material; the energy balance is defined
    for ``linear`` only (ValueError otherwise).  ``dt_check_every = S > 0`` (a nonlinear material on the whole mesh only,
    ValueError otherwise): the run is split into calls of ``S`` steps - the stepper is bit-equal under any split - and after
    each, the last included, :meth:`OperatorStepper.stable_time_step` measures the limit at the current state; the report
    gains ``dt_check``: ``every``, ``n_checks``, ``dt_crit_min`` and the step count ``dt_crit_min_step`` at which it was seen,
    ``dt_over_dt_crit_max`` and ``first_exceeded_step`` (the step count of the first check with ``dt > dt_crit``, -1: never).
    ``dt`` is not changed during the run - unless ``dt_follow`` is ``"certified"`` or ``"anchored"`` (a nonlinear material on
    the whole mesh without the energy balance, ValueError otherwise): then :meth:`OperatorStepper.follow_time_step` checks the
    step before step 0 and after every ``dt_follow_every`` steps and changes it by that method's rule, ``dt_check`` reports
    against the ``dt`` in use at each check, the report gains ``dt_follow`` (``mode``, ``every``, ``n_checks``, ``n_changes``,
    ``dt_first``, ``dt_min``, ``dt_last``, ``omega_bound_0``, ``omega_bound_max`` and ``bound_over_lanczos_0``, the bound at ``u = 0``
    over the Lanczos ``omega_max`` of the linear operator) and the return value a third member, ``{"t", "step", "dt"}``: the time
    of every saved column - they are no longer equidistant - and the ``(step, dt)`` list of the run, the first entry the step
    it began with.  Without ``dt_follow`` the report and the return value are what they were, key for key."""
    import torch

    mat = _lib.material_id(material)
    material = str(material).replace("-", "_")
    dt_follow_every = int(dt_follow_every or 0)
    if dt_follow is not None:
        if dt_follow not in ("certified", "anchored"):
            raise ValueError(f"dt_follow must be None, 'certified' or 'anchored', not {dt_follow!r}")
        if dt_follow_every < 1:
            raise ValueError("dt_follow_every must be >= 1")
        if mat == 0:
            raise ValueError("following the time step is for a nonlinear material: the linear operator's limit does not move")
        if epart is not None:
            raise ValueError("following the time step is not defined for a partition: a rank holds only its share of the internal force")
        if energy_every:
            raise ValueError("following the time step is not defined with the energy balance: its identity assumes one dt")
    if mat != 0 and energy_every:
        raise ValueError("the energy balance is defined for the linear material only: its identity needs a symmetric constant K")
    dt_check_every = int(dt_check_every or 0)
    if dt_check_every < 0:
        raise ValueError("dt_check_every must be >= 0")
    if dt_check_every and mat == 0:
        raise ValueError("the time-step check is for a nonlinear material: the linear operator's limit does not move")
    if dt_check_every and epart is not None:
        raise ValueError("the time-step check is not defined for a partition: a rank's operator is only its share of the tangent")

    from . import fem_setup as fs
    from .modal import ModalOperator, stable_time_step_operator

    points = np.ascontiguousarray(points, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    if epart is not None:
        return _run_dynamics_parts(points, cells, dirichlet_nodes, epart, n_steps, save_every, E, nu, rho, fz, alpha, gamma, device,
                                   energy_every, material)
    n_rows = -(-int(n_steps) // int(energy_every)) if energy_every else 0
    lmd, mu = fs.lame(E, nu)
    with ModalOperator(points, cells, fs.node_to_dof(dirichlet_nodes), lmd, mu, rho, device) as op:
        mass = op.lumped_mass()
        ts = stable_time_step_operator(op, mass, gamma)
        n_cols = int(n_steps / save_every)
        with OperatorStepper(op, mass, op.load((0.0, -fz, -fz)), ts["dt"], alpha, ramp=True, material=material) as st:
            traj = st.record(n_cols, save_every) if n_cols > 0 else None
            rows = st.record_energy(n_rows, energy_every) if n_rows > 0 else None
            if dt_follow is not None:
                # follow before step 0 and after every dt_follow_every steps, measure after every dt_check_every steps
                checks, follows, done, total = [], [], 0, int(n_steps)
                while done < total:
                    if done % dt_follow_every == 0:
                        follows.append(st.follow_time_step(dt_follow, gamma, omega_linear=ts["omega_max"]))
                    stops = [total, (done // dt_follow_every + 1) * dt_follow_every]
                    if dt_check_every:
                        stops.append((done // dt_check_every + 1) * dt_check_every)
                    n = min(stops) - done
                    st.step(n)
                    done += n
                    if dt_check_every and (done % dt_check_every == 0 or done == total):
                        checks.append((done, st.stable_time_step(gamma)))
            elif dt_check_every:
                checks, done = [], 0
                while done < int(n_steps):
                    n = min(dt_check_every, int(n_steps) - done)
                    st.step(n)
                    done += n
                    checks.append((done, st.stable_time_step(gamma)))
            else:
                st.step(n_steps)
            d0, _, tn = st.state()
            inverted, first_inverted = st.inverted()
            store = traj.cpu().numpy() if traj is not None else np.zeros((op.n_dof, 0))
            table = rows.cpu().numpy() if rows is not None else np.zeros((0, 5))
        d = d0.cpu().numpy().reshape(-1, 3)
        n_vert = int(cells[:, :4].max()) + 1 if len(cells) else 0
        tip = np.nonzero(np.abs(points[:n_vert, 0] - points[:, 0].max()) < 1e-9)[0]
        rule = reference_rule_dt(points, cells, E, nu, rho, gamma)
        report = {"order": op.order, "n_nodes": op.n_nodes, "n_elems": op.n_elems,
                  "n_free_dofs": int(op.free.sum().item()), "dt": ts["dt"], "dt_crit": ts["dt_crit"],
                  "dt_reference_rule": rule, "ratio": rule / ts["dt_crit"], "omega_max": ts["omega_max"], "steps": int(n_steps),
                  "tn": tn, "max_abs_d": float(np.abs(d).max()), "tip_deflection": float(-d[tip, 1].mean())}
        if mat != 0:
            report.update(material=material, inverted=inverted, first_inverted_step=first_inverted)
        if dt_check_every:
            report["dt_check"] = dt_check_report(checks, dt_check_every)
        if dt_follow is not None:
            omega_0 = op.tangent_bound(None, "linear")["omega_max"]
            report["dt_follow"], times = dt_follow_report(follows, dt_follow, dt_follow_every, ts["dt"], omega_0, ts["omega_max"],
                                                          int(n_steps), int(save_every), n_cols)
    torch.cuda.synchronize(device)
    if dt_follow is not None:
        return store, report, times
    if energy_every:
        report["energy"] = energy_report(table)
        return store, report, table
    return store, report


def run_dynamics_newmark(points, cells, dirichlet_nodes, n_steps, save_every=1, E=1e6, nu=0.3, rho=1.0, fz=0.5, alpha=0.5,
                         gamma=0.9, device=0, material="linear", dt_factor=10.0, newton_tol=1e-10):
    """:func:`run_dynamics` of the whole mesh with the implicit stepper (:class:`ImplicitStepper`) in the place of the
    explicit one: same handle, clamp, lumped mass, ramped load ``(0, -fz, -fz)`` and ``alpha``, but ``dt = dt_factor * 2/omega_max``
    of the linear operator - a multiple of the explicit limit, chosen for the physics.  Returns ``(store, report)`` with the
    explicit run's layout and keys (``dt_crit`` is still the explicit limit; with a nonlinear material ``inverted`` is 1 and
    ``first_inverted_step`` the failed step when a trial state held an inverted element, else 0 and -1) plus ``scheme``,
    ``dt_factor``, ``newton_iterations``, ``cg_iterations``, ``converged`` and ``failed_step`` (-1: none; else the index of the step
    that was not accepted - the run stops there and the columns from it on stay 0)."""
    import torch

    from . import fem_setup as fs
    from .modal import ModalOperator, stable_time_step_operator

    mat = _lib.material_id(material)
    material = str(material).replace("-", "_")
    if not (dt_factor > 0 and newton_tol > 0):
        raise ValueError("need dt_factor > 0 and newton_tol > 0")
    points = np.ascontiguousarray(points, dtype=np.float64)
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    lmd, mu = fs.lame(E, nu)
    with ModalOperator(points, cells, fs.node_to_dof(dirichlet_nodes), lmd, mu, rho, device) as op:
        mass = op.lumped_mass()
        ts = stable_time_step_operator(op, mass, gamma)
        dt = float(dt_factor) * ts["dt_crit"]
        n_cols = int(n_steps / save_every)
        with ImplicitStepper(op, mass, op.load((0.0, -fz, -fz)), dt, alpha, ramp=True, material=material) as st:
            st.set_option("tol", newton_tol)
            traj = st.record(n_cols, save_every) if n_cols > 0 else None
            info = st.step(n_steps)
            d0, _, _, tn = st.state()
            store = traj.cpu().numpy() if traj is not None else np.zeros((op.n_dof, 0))
        d = d0.cpu().numpy().reshape(-1, 3)
        n_vert = int(cells[:, :4].max()) + 1 if len(cells) else 0
        tip = np.nonzero(np.abs(points[:n_vert, 0] - points[:, 0].max()) < 1e-9)[0]
        rule = reference_rule_dt(points, cells, E, nu, rho, gamma)
        failed = -1 if info["converged"] else info["steps_done"]
        report = {"order": op.order, "n_nodes": op.n_nodes, "n_elems": op.n_elems,
                  "n_free_dofs": int(op.free.sum().item()), "dt": dt, "dt_crit": ts["dt_crit"],
                  "dt_reference_rule": rule, "ratio": rule / ts["dt_crit"], "omega_max": ts["omega_max"], "steps": int(n_steps),
                  "tn": tn, "max_abs_d": float(np.abs(d).max()), "tip_deflection": float(-d[tip, 1].mean())}
        if mat != 0:
            inv = info["reason"] == 3
            report.update(material=material, inverted=int(inv), first_inverted_step=failed if inv else -1)
        report.update(scheme="newmark", dt_factor=float(dt_factor), newton_iterations=info["newton_iterations"],
                      cg_iterations=info["cg_iterations"], converged=info["converged"], failed_step=failed)
    torch.cuda.synchronize(device)
    return store, report


def dt_check_report(checks, every):
    """What ``drivers dynamics --dt-check-every`` prints of ``[(steps done, OperatorStepper.stable_time_step())]``."""
    out = {"every": int(every), "n_checks": len(checks), "dt_crit_min": None, "dt_crit_min_step": -1,
           "dt_over_dt_crit_max": None, "first_exceeded_step": -1}
    if checks:
        step, low = min(checks, key=lambda c: c[1]["dt_crit"])
        out.update(dt_crit_min=low["dt_crit"], dt_crit_min_step=step,
                   dt_over_dt_crit_max=max(c[1]["dt_over_dt_crit"] for c in checks),
                   first_exceeded_step=next((s for s, c in checks if c["dt_over_dt_crit"] > 1.0), -1))
    return out


def dt_follow_report(follows, mode, every, dt_created, omega_bound_0, omega_lanczos_0, n_steps, save_every, n_cols):
    """What ``drivers dynamics --dt-follow`` prints of the records ``[(step, Omega, target, dt)]`` of
    :meth:`OperatorStepper.follow_time_step`, and the times of the run: ``(report, {"t": (n_cols,), "step": (k,), "dt": (k,)})``
    with ``t[c]`` the time of saved column ``c`` (the state after step ``c * save_every``, the ramp's clock starting at 0) and
    ``(step[j], dt[j])`` the step in use from step ``step[j]`` on, the first entry the step of the first check."""
    dts = [r[3] for r in follows]
    steps = np.array([r[0] for r in follows], dtype=np.int64)
    per_step = np.zeros(int(n_steps))
    for j, r in enumerate(follows):
        per_step[r[0]:(follows[j + 1][0] if j + 1 < len(follows) else int(n_steps))] = r[3]
    after = np.cumsum(per_step)                                       # the time after step i
    t = after[np.arange(int(n_cols), dtype=np.int64) * int(save_every)] if n_cols > 0 else np.zeros(0)
    changed = [0] + [j for j in range(1, len(dts)) if dts[j] != dts[j - 1]]   # the first check, then every check that moved dt
    report = {"mode": mode, "every": int(every), "n_checks": len(follows),
              "n_changes": sum(a != b for a, b in zip([dt_created] + dts[:-1], dts)),
              "dt_first": dts[0] if dts else None, "dt_min": min(dts) if dts else None, "dt_last": dts[-1] if dts else None,
              "omega_bound_0": omega_bound_0, "omega_bound_max": max((r[1] for r in follows), default=None),
              "bound_over_lanczos_0": omega_bound_0 / omega_lanczos_0}
    keep = np.array(changed, dtype=np.int64)
    return report, {"t": t, "step": steps[keep] if dts else steps, "dt": np.array(dts)[keep] if dts else np.zeros(0)}


def _run_dynamics_parts(points, cells, dirichlet_nodes, epart, n_steps, save_every, E, nu, rho, fz, alpha, gamma, device,
                        energy_every=0, material="linear"):
    import torch

    from . import fem_setup as fs
    from .modal import ModalOperator

    n_cols = int(n_steps / save_every)
    with OperatorPartition(points, cells, dirichlet_nodes, epart, None, E, nu, rho, fz, alpha, gamma, True, device,
                           material=material) as part:
        trajs = [r.stepper.record(n_cols, save_every) if n_cols > 0 else None for r in part.ranks]
        n_rows = -(-int(n_steps) // int(energy_every)) if energy_every else 0
        if n_rows > 0:
            part.record_energy(n_rows, energy_every)
        part.step_synced(n_steps)
        table = part.energy().cpu().numpy() if n_rows > 0 else np.zeros((0, 5))
        d = part.gather("d0").cpu().numpy().reshape(-1, 3)
        tn = part.tn
        inverted, first_inverted = part.inverted()
        store = np.zeros((part.n_dof, n_cols))
        for r, traj in reversed(list(zip(part.ranks, trajs))):
            if traj is not None:
                store[r.global_dof.cpu().numpy()] = traj.cpu().numpy()
        ts, order = part.time_step, part.order
        shared = [len(r.layout.shared_local) for r in part.ranks]
        n_global_shared, parts = len(part.global_shared), part.n_parts
    with ModalOperator(points, cells, fs.node_to_dof(dirichlet_nodes), *fs.lame(E, nu), rho, device) as op:
        n_free = int(op.free.sum().item())
    n_vert = int(cells[:, :4].max()) + 1 if len(cells) else 0
    tip = np.nonzero(np.abs(points[:n_vert, 0] - points[:, 0].max()) < 1e-9)[0]
    rule = reference_rule_dt(points, cells, E, nu, rho, gamma)
    report = {"order": order, "n_nodes": len(points), "n_elems": len(cells), "n_free_dofs": n_free, "dt": ts["dt"],
              "dt_crit": ts["dt_crit"], "dt_reference_rule": rule, "ratio": rule / ts["dt_crit"], "omega_max": ts["omega_max"],
              "steps": int(n_steps), "tn": tn, "max_abs_d": float(np.abs(d).max()), "tip_deflection": float(-d[tip, 1].mean()),
              "parts": parts, "n_global_shared": n_global_shared, "shared_per_rank": shared}
    if _lib.material_id(material) != 0:
        report.update(material=material, inverted=inverted, first_inverted_step=first_inverted)
    torch.cuda.synchronize(device)
    if energy_every:
        report["energy"] = energy_report(table)
        return store, report, table
    return store, report
