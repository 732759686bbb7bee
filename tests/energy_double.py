"""NumPy double of the energy balance of the operator stepper (``saa_operator_stepper_set_energy``, ``csrc/saa_opstep.hip``):
the five columns ``T_{n+1/2}, U_{n+1/2}, U_n, W, D`` from the states of the doubles of the time loop -
``p2_dynamics_double.run`` for the whole mesh, ``p2_partition_double.PartitionDouble`` for a partition - in plain float64
sums, with ``K d`` from the double's own dense operator and, per rank, the shares under the lowest-holder ownership rule.

A dof is live when it is free and its node has an element (on the rank); only live dofs are summed.  Order 1 is the same
loop on the dense ``K`` of the linear element (``oracle.fem_oracle.assemble_local_stiffness``, Dirichlet rows and columns
zeroed) with the row-sum mass; a node without elements gets the mass 1 here so that the loop never divides by zero - it is
not live and stays at rest."""
from __future__ import annotations

import numpy as np

import p2_double as p2
import p2_dynamics_double as dyn
import p2_partition_double as pd

from oracle import fem_oracle as fo
from synchronization_avoiding_algorithms_amd import fem_setup as fs


def dense_k(points, cells, dirichlet, lmd, mu, rho=1.0):
    """Dense masked ``K`` of 4- or 10-column ``cells``."""
    cells = np.asarray(cells)
    if cells.shape[1] == 10:
        return p2.assemble(points, cells, dirichlet, lmd, mu, rho)[0]
    n = len(points)
    K = np.asarray(fo.assemble_local_stiffness(np.arange(n), cells.astype(np.int64), np.asarray(points, dtype=np.float64), lmd,
                                               mu).todense())
    free = np.ones(3 * n)
    free[np.asarray(dirichlet, dtype=np.int64)] = 0.0
    return K * free[:, None] * free[None, :]


def live_dofs(n_nodes, cells, dirichlet):
    live = np.zeros(n_nodes, dtype=bool)
    live[np.unique(np.asarray(cells))] = True
    live = np.repeat(live, 3)
    live[np.asarray(dirichlet, dtype=np.int64)] = False
    return live


def problem(points, cells, dirichlet, lmd, mu, rho, fz):
    """``dict(K, mass, load, live)`` of either order: HRZ mass and consistent load for 10 columns, row-sum mass ``rho V / 4``
    and load ``f V / 4`` for 4 (mass 1 at a node without elements)."""
    cells = np.asarray(cells)
    K = dense_k(points, cells, dirichlet, lmd, mu, rho)
    if cells.shape[1] == 10:
        mass, load = dyn.hrz_mass(points, cells, rho), p2.load(points, cells, dirichlet, (0.0, -fz, -fz))
    else:
        mass, load = (a.ravel().copy() for a in fs.lumped_mass_and_load(np.asarray(points, dtype=np.float64), cells, rho, fz))
        mass[mass == 0.0] = 1.0
    return dict(K=K, mass=mass, load=load, live=live_dofs(len(points), cells, dirichlet))


def five(s, m, f, d0, dn, d1, dt, alpha, lam, mass_terms, half, now):
    """One step's ``(T, U_{n+1/2}, U_n, dW, dD)``: boolean masks say which dofs enter the terms with ``m`` or ``f``, the
    cross form and ``U_n``."""
    v, w = (d1 - d0) / dt, d1 - dn
    return np.array([0.5 * np.sum((m * v * v)[mass_terms]), 0.5 * np.sum((d1 * s)[half]), 0.5 * np.sum((d0 * s)[now]),
                     lam * np.sum((f * w / 2.0)[mass_terms]), alpha / (4.0 * dt) * np.sum((m * w * w)[mass_terms])])


def accumulate(steps):
    """``(n, 5)`` per-step sums -> rows: columns 3 and 4 become the running ``W_{n+1}``, ``D_{n+1}``."""
    rows = np.array(steps, dtype=np.float64).reshape(-1, 5)
    rows[:, 3] = np.cumsum(rows[:, 3])
    rows[:, 4] = np.cumsum(rows[:, 4])
    return rows


def balance(rows):
    b = rows[:, 0] + rows[:, 1] - rows[:, 3] + rows[:, 4]
    return b - b[0]


def scale(rows):
    return max(rows[:, 3].max(), (rows[:, 0] + rows[:, 1]).max())


def run_whole(K, mass, load, dirichlet, live, dt, alpha, ramp, nsteps, d0=None, dn=None, tn=0.0):
    """``p2_dynamics_double.run`` with the energy rows of every step: ``(rows (nsteps, 5), (d0, dn, tn))``."""
    n = len(mass)
    st = dict(d0=np.zeros(n) if d0 is None else np.array(d0, dtype=np.float64),
              dn=np.zeros(n) if dn is None else np.array(dn, dtype=np.float64), tn=tn)
    steps = []

    def record(i, d1):
        lam = min(st["tn"], 1.0) if ramp else 1.0
        steps.append(five(K @ st["d0"], mass, load, st["d0"], st["dn"], d1, dt, alpha, lam, live, live, live))
        st["dn"], st["d0"] = st["d0"], d1.copy()
        st["tn"] += dt

    out = dyn.run(K, mass, load, dirichlet, dt, alpha, ramp, nsteps, d0=d0, dn=dn, tn=tn, record=record)
    return accumulate(steps), out


class LinearRank(pd.Rank):
    """``p2_partition_double.Rank`` with the linear element's ``K``."""

    def __init__(self, points, layout, n_global_shared, mass, load, lmd, mu, rho):
        self.layout = layout
        self.K = dense_k(points[layout.nodes], layout.cells_local, layout.dirichlet_dofs, lmd, mu)
        dof = np.asarray(layout.local_dof, dtype=np.int64)
        self.dof = dof
        self.mass, self.load = np.asarray(mass)[dof], np.asarray(load)[dof]
        self.dd = np.asarray(layout.dirichlet_dofs, dtype=np.int64)
        self.loc = np.asarray(layout.loc_dof_shared, dtype=np.int64)
        self.gd = (3 * np.asarray(layout.shared_slots, dtype=np.int64)[:, None] + np.arange(3)[None, :]).ravel()
        self.d0, self.dn = np.zeros(len(dof)), np.zeros(len(dof))


def ownership(layouts, n_global_shared):
    """Per rank, one flag per shared node in table order: the rank is the node's lowest holder."""
    owner = np.full(n_global_shared, len(layouts))
    for lay in layouts:
        owner[lay.shared_slots] = np.minimum(owner[lay.shared_slots], lay.rank)
    return [owner[lay.shared_slots] == lay.rank for lay in layouts]


class EnergyPartitionDouble(pd.PartitionDouble):
    """``PartitionDouble`` of either order whose steps also append every rank's share of the energy sums to
    ``self.steps[rank]``; ``rows(rank)`` / ``total()`` turn them into rows."""

    def __init__(self, points, layouts, global_shared, mass, load, lmd, mu, rho, dt, alpha, ramp=True):
        if np.asarray(layouts[0].cells_local).shape[1] == 10:
            super().__init__(points, layouts, global_shared, mass, load, lmd, mu, rho, dt, alpha, ramp)
        else:
            self.n_global_shared = len(global_shared)
            self.ranks = [LinearRank(np.asarray(points), lay, self.n_global_shared, mass, load, lmd, mu, rho) for lay in layouts]
            self.dt, self.alpha, self.ramp, self.tn = float(dt), float(alpha), bool(ramp), 0.0
            self.n_dof = 3 * len(points)
        self.steps = [[] for _ in self.ranks]
        for r, own in zip(self.ranks, ownership(layouts, self.n_global_shared)):
            r.live = np.ones(len(r.dof), dtype=bool)                # every node of a rank has an element of the rank
            r.live[r.dd] = False
            r.shared = np.zeros(len(r.dof), dtype=bool)
            r.shared[r.loc] = True
            r.own = np.ones(len(r.dof), dtype=bool)                  # the rank counts the dof's mass and load terms
            r.own[r.loc] = np.repeat(own, 3)

    def _lam(self):
        return min(self.tn, 1.0) if self.ramp else 1.0

    def step_synced(self, n=1, hists=None, row0=0):
        for k in range(n):
            partial = [r.K @ r.d0 for r in self.ranks]
            before = [(r.d0, r.dn) for r in self.ranks]
            lam = self._lam()
            super().step_synced(1, hists, row0 + k)
            iface = np.zeros(3 * self.n_global_shared)
            for r, f in zip(self.ranks, partial):
                iface[r.gd] += f[r.loc]
            for i, (r, f, (d0, dn)) in enumerate(zip(self.ranks, partial, before)):
                full = f.copy()
                full[r.loc] = iface[r.gd]
                e = five(full, r.mass, r.load, d0, dn, r.d0, self.dt, self.alpha, lam, r.live & r.own, r.live & r.own,
                         np.zeros_like(r.live))
                e[2] = 0.5 * np.sum((d0 * f)[r.live])                # U_n from the partial force on every holder
                self.steps[i].append(e)

    def step_predicted(self, n, tables, table_row0=0, hists=None, hist_row0=0):
        for k in range(n):
            partial = [r.K @ r.d0 for r in self.ranks]
            before = [(r.d0, r.dn) for r in self.ranks]
            lam = self._lam()
            super().step_predicted(1, tables, table_row0 + k, hists, hist_row0 + k)
            for i, (r, f, (d0, dn)) in enumerate(zip(self.ranks, partial, before)):
                self.steps[i].append(five(f, r.mass, r.load, d0, dn, r.d0, self.dt, self.alpha, lam, r.live & r.own, r.live, r.live))

    def rows(self, rank):
        return accumulate(self.steps[rank])

    def total(self):
        return sum(self.rows(i) for i in range(len(self.ranks)))

    @classmethod
    def from_epart(cls, points, cells, dirichlet_nodes, epart, n_parts, mass, load, lmd, mu, rho, dt, alpha, ramp=True):
        layouts, gs = fs.build_layouts(cells, epart, n_parts, len(points), dirichlet_nodes)
        return cls(points, layouts, gs, mass, load, lmd, mu, rho, dt, alpha, ramp)
