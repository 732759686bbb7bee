"""fp64 reference of the kernels behind the training pass (``lstm_rec_*``, ``lstm_cell_*``, ``train_stats_*`` of
csrc/saa_predictor.hip), the case families that take them to their edges, and the bar they are held to.  Shared by
tests/test_training_extended.py (CPU) and tests/test_gpu_training_edges.py.  Lives under tests/: the product never imports
it.  Plain PyTorch on the CPU, fp64 unless said otherwise; the statistics in ``np.longdouble``.

The reference.  :func:`recurrence` is ``gates_t = pre_t + h_{t-1} W^T;  i, f, g, o = s, s, tanh, s;  c_t = f c_{t-1} + i g;
h_t = o tanh(c_t)`` step by step, :func:`cell` its pointwise part; gradients come from autograd on leaves of the working
type (of ``sum(H wh) + sum(c_T wc)`` with seeded weights, so that every output has a gradient).  The fp64 run takes the fp32
inputs widened exactly.  ``form`` selects how the gates are activated:

* ``"tanh"``: ``torch.sigmoid`` / ``torch.tanh`` - the reference;
* ``"two_sigmoid"``: ``tanh v = 2 s(2v) - 1``, what ``lstm_rec_forward_kernel`` did before: 6e-8 of ABSOLUTE error on the
  tanh gate whatever ``|v|`` is - only here to prove that the bar can fail;
* ``"kernel"``: what the kernel does now, ``tanh`` on the tanh gate and the sigmoid spelled as ``sigmoid_f32`` spells it,
  ``1 / (1 + exp(-x))`` (``exp`` overflows to inf past 88.7 and the quotient is an exact 0: no NaN).  In both of these the
  derivatives come from the stored activations, ``s (1 - s)`` and ``1 - t^2``, as in the backward kernels.

The error measure, per output field: ``err = max|y - r| / max|r|`` against the fp64 result ``r``.

The bar: ``err_kernel <= 8 env`` (``KERNEL_FACTOR``, a condition and not a measurement: it allows another summation order
and the device's own ``expf`` / ``tanhf``).  ``env``, per case and field, is the ``err`` of the fp32 ``"tanh"`` restatement on
the CPU - what fp32 costs the reference's own formulation - as the larger of ``N_DRAWS`` seeded input draws (draw 0 is the one
the GPU test feeds the kernels).  The bar is only meaningful where ``env <= ENV_MAX`` (with ``W`` of scale 1.0 at width 100 the
recurrence is chaotic and fp32 itself is 5e-3 off: no such family here), where the fp32 restatement of the kernel's own form
stays within ``2 env``, and where a wrong reference shows: the fp64 recurrence with the last column of ``W`` zeroed, and the
one whose last processed step reads its neighbour's ``pre`` row (the kernels' one-step-ahead clamp gone wrong), each have to
move ``H`` by ``SENSITIVITY * bar`` at least.  tests/test_training_extended.py asserts all of this on every family.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

KERNEL_FACTOR, STABLE_FACTOR, ENV_MAX, N_DRAWS, SENSITIVITY = 8.0, 2.0, 1e-5, 3, 100.0
TOL = 1e-12                    # the project's bar for fp64 sums (tests/test_gpu_p2_stress.py)

#: recurrence families: name -> (B, T, scale of pre, scale of W, scale of h0 / c0); each at widths 50 and 100, both directions
REC_FAMILIES = {
    "std": (7, 20, 0.5, 0.2, 0.3),
    "small": (7, 20, 1e-4, 0.2, 1e-4),            # small signal: the tanh gate's RELATIVE accuracy near zero
    "small100": (7, 20, 1e-3, 0.1, 1e-3),
    "saturated": (7, 20, 30.0, 0.2, 0.3),         # saturated gates
    "saturated100": (7, 20, 100.0, 0.2, 0.3),     # past the overflow of fp32 exp (88.7)
    "long": (3, 200, 0.5, 0.2, 0.3),
    "T1": (1, 1, 0.5, 0.2, 0.3),                  # T = 1, 2: where the kernels' look-ahead clamps
    "T2": (1, 2, 0.5, 0.2, 0.3),
    "B300": (300, 20, 0.5, 0.2, 0.3),             # a grid of 300 workgroups
    # 500 and 520 rows: either side of training._DW_ONE_PRODUCT_ROWS, where the weight gradient goes from one product
    # over all rows to one per batch row (B300 is far inside the second)
    "B25": (25, 20, 0.5, 0.2, 0.3),
    "B26": (26, 20, 0.5, 0.2, 0.3),
}
SMALL_SIGNAL = ("small", "small100")
WIDTHS = (50, 100)
#: (h0 given, c0 given): both, neither, c0 only (what training._decode_folded passes), h0 only
STATES = {"both": (True, True), "neither": (False, False), "c0_only": (False, True), "h0_only": (True, False)}

#: cell families: the (B, D) of tests/test_training.py (B D at 255, 256, 257 and above 2^20) x the scale of the gates
CELL_SHAPES = ((10, 100), (3, 7), (1, 1), (5, 51), (2, 128), (1, 257), (1025, 1024))
CELL_SCALES = (1.0, 30.0, 100.0)
#: a single saturated element is no case: its gradients are 1e-13 and below, fp32 flushes what fp64 keeps (env of 5e-4 in
#: dgates at scale 30 and of 1.0 in dc_prev at scale 100), and ``max|r|`` needs an unsaturated element to mean something
CELL_CASES = tuple((B, D, s) for B, D in CELL_SHAPES for s in CELL_SCALES if not (B * D == 1 and s > 1.0))

CELL_FIELDS = ("h", "c", "dgates", "dc_prev")


# ----------------------------------------------------------------------------------------------------------------------
# Activations and the two operations
# ----------------------------------------------------------------------------------------------------------------------

class _FromOutput(torch.autograd.Function):
    """An activation whose derivative is formed from its stored OUTPUT, as the backward kernels do from the activations
    the forward kept: ``s (1 - s)`` and ``1 - t^2`` (autograd through ``1 / (1 + exp(-x))`` would give ``inf * 0`` at
    ``x = -100``, which no kernel computes)."""

    @staticmethod
    def forward(ctx, x, value, is_tanh):
        ctx.save_for_backward(value)
        ctx.is_tanh = is_tanh
        return value.clone()

    @staticmethod
    def backward(ctx, d):
        y, = ctx.saved_tensors
        return d * ((1.0 - y * y) if ctx.is_tanh else y * (1.0 - y)), None, None


def _sigmoid(x, form):
    if form in ("tanh", "two_sigmoid"):
        return torch.sigmoid(x)
    if form == "kernel":
        return _FromOutput.apply(x, 1.0 / (1.0 + torch.exp(-x.detach())), False)
    raise ValueError(form)


def _tanh(v, form):
    if form in ("tanh", "kernel"):
        return torch.tanh(v)
    if form == "two_sigmoid":
        return _FromOutput.apply(v, 2.0 * torch.sigmoid(2.0 * v.detach()) - 1.0, True)
    raise ValueError(form)


def recurrence(pre, W, h0, c0, T, reverse, dtype=torch.float64, form="tanh"):
    """Every ``h_t`` as ``(B, T, H)`` and the final ``c`` of the recurrence over ``pre`` ``(B, T, 4H)``; ``h0`` / ``c0`` may be
    None (zero).  ``form`` activates the gates; the cell's own ``tanh(c_t)`` is ``torch.tanh`` in every form (``tanhf`` in
    the kernels)."""
    B, Hd = pre.shape[0], W.shape[1]
    pre, W = pre.to(dtype), W.to(dtype)
    h = h0.to(dtype) if h0 is not None else torch.zeros(B, Hd, dtype=dtype)
    c = c0.to(dtype) if c0 is not None else torch.zeros(B, Hd, dtype=dtype)
    seq = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gi, gf, gg, go = (pre[:, t, :] + h @ W.t()).chunk(4, dim=1)
        c = _sigmoid(gf, form) * c + _sigmoid(gi, form) * _tanh(gg, form)
        h = _sigmoid(go, form) * torch.tanh(c)
        seq[t] = h
    return torch.stack(seq, dim=1), c


def cell(gates, c_prev, dtype=torch.float64):
    """``(h, c)`` of one step's pointwise part from the pre-activations ``(B, 4D)`` in PyTorch's gate order."""
    gi, gf, gg, go = gates.to(dtype).chunk(4, dim=1)
    c = torch.sigmoid(gf) * c_prev.to(dtype) + torch.sigmoid(gi) * torch.tanh(gg)
    return torch.sigmoid(go) * torch.tanh(c), c


def err(y, r):
    """``max|y - r| / max|r|``; inf for a NaN or an inf in ``y``.  A reference that is zero everywhere (the weight gradient
    of a single step from a zero ``h``) leaves ``max|y|``: the fp32 restatement gives exact zeros there, so ``env`` is 0
    and the bar asks the kernel for exact zeros too."""
    y, r = torch.as_tensor(y).detach().double().cpu(), torch.as_tensor(r).detach().double().cpu()
    if not bool(torch.isfinite(y).all()):
        return float("inf")
    scale = float(r.abs().max())
    return float((y - r).abs().max()) / (scale if scale > 0 else 1.0)


# ----------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------

def _generator(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rec_inputs(family, width, reverse, draw=0):
    """The fp32 inputs of a recurrence case (CPU): ``pre, W, h0, c0`` and the weights ``wh, wc`` of the scalar whose
    gradients are compared.  The state combinations share them (an absent state is simply not passed)."""
    B, T, s_pre, s_w, s_state = REC_FAMILIES[family]
    g = _generator("rec", family, width, bool(reverse), draw)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)  # noqa: E731
    return {"pre": rn(B, T, 4 * width) * s_pre, "W": rn(4 * width, width) * s_w, "h0": rn(B, width) * s_state,
            "c0": rn(B, width) * s_state, "wh": rn(B, T, width), "wc": rn(B, width), "T": T, "reverse": bool(reverse)}


def rec_outputs(inp, state, dtype=torch.float64, form="tanh", mutate=None):
    """``H``, ``c``, ``dpre``, ``dW``, ``dh0``, ``dc0`` of the recurrence on ``inp`` in ``dtype`` (``dh0`` / ``dc0`` only where
    that state is given).
    ``mutate``: ``"w_column"`` zeroes the last column of ``W``, ``"pre_neighbour"`` gives the last processed step the
    ``pre`` row of the step before it - two wrong references for the sensitivity condition (forward only)."""
    has_h0, has_c0 = STATES[state]
    T, reverse = inp["T"], inp["reverse"]
    pre, W = inp["pre"].to(dtype), inp["W"].to(dtype)
    if mutate == "w_column":
        W = W.clone()
        W[:, -1] = 0.0
    elif mutate == "pre_neighbour":
        pre = pre.clone()
        last, before = (0, 1) if reverse else (T - 1, T - 2)
        pre[:, last, :] = pre[:, before, :]
    elif mutate is not None:
        raise ValueError(mutate)
    leaves = {"dpre": pre.requires_grad_(), "dW": W.requires_grad_()}
    if has_h0:
        leaves["dh0"] = inp["h0"].to(dtype).requires_grad_()
    if has_c0:
        leaves["dc0"] = inp["c0"].to(dtype).requires_grad_()
    H, c = recurrence(pre, W, leaves.get("dh0"), leaves.get("dc0"), T, reverse, dtype, form)
    out = {"H": H.detach(), "c": c.detach()}
    if mutate is None:
        grads = torch.autograd.grad((H * inp["wh"].to(dtype)).sum() + (c * inp["wc"].to(dtype)).sum(), list(leaves.values()))
        out.update(zip(leaves, grads))
    return out


def cell_inputs(B, D, scale, draw=0):
    g = _generator("cell", B, D, scale, draw)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)  # noqa: E731
    return {"gates": rn(B, 4 * D) * scale, "c_prev": rn(B, D), "wh": rn(B, D), "wc": rn(B, D)}


def cell_outputs(inp, dtype=torch.float64):
    gates, c_prev = inp["gates"].to(dtype).requires_grad_(), inp["c_prev"].to(dtype).requires_grad_()
    h, c = cell(gates, c_prev, dtype)
    dgates, dc_prev = torch.autograd.grad((h * inp["wh"].to(dtype)).sum() + (c * inp["wc"].to(dtype)).sum(), (gates, c_prev))
    return {"h": h.detach(), "c": c.detach(), "dgates": dgates, "dc_prev": dc_prev}


def errors(got, want):
    return {k: err(got[k], want[k]) for k in want}


@functools.lru_cache(maxsize=None)
def rec_reference(family, width, reverse, state):
    """The fp64 fields of draw 0 (computed once, shared, never modified)."""
    return rec_outputs(rec_inputs(family, width, reverse), state)


@functools.lru_cache(maxsize=None)
def rec_env(family, width, reverse, state):
    """field -> the ``err`` of the fp32 ``"tanh"`` restatement, the larger of ``N_DRAWS`` draws."""
    env = {}
    for draw in range(N_DRAWS):
        inp = rec_inputs(family, width, reverse, draw)
        want = rec_reference(family, width, reverse, state) if draw == 0 else rec_outputs(inp, state)
        for k, v in errors(rec_outputs(inp, state, torch.float32), want).items():
            env[k] = max(env.get(k, 0.0), v)
    return env


@functools.lru_cache(maxsize=None)
def cell_reference(B, D, scale):
    return cell_outputs(cell_inputs(B, D, scale))


@functools.lru_cache(maxsize=None)
def cell_env(B, D, scale):
    env = {}
    for draw in range(N_DRAWS):
        inp = cell_inputs(B, D, scale, draw)
        want = cell_reference(B, D, scale) if draw == 0 else cell_outputs(inp)
        for k, v in errors(cell_outputs(inp, torch.float32), want).items():
            env[k] = max(env.get(k, 0.0), v)
    return env


def check_bar(got, want, env, label):
    """Print ``err``, ``env`` and their ratio per field, then hold every field to ``KERNEL_FACTOR * env``."""
    e = errors(got, want)
    ratio = {k: e[k] / env[k] if env[k] > 0 else (0.0 if e[k] == 0 else float("inf")) for k in e}
    print(label, "  ".join(f"{k}: err {e[k]:.2e} env {env[k]:.2e} ratio {ratio[k]:.2f}" for k in e))
    bad = {k: (e[k], env[k]) for k in e if not e[k] <= KERNEL_FACTOR * env[k]}
    assert not bad, (label, bad)
    return e


# ----------------------------------------------------------------------------------------------------------------------
# The training figures (DNN_tools.py:144-155)
# ----------------------------------------------------------------------------------------------------------------------

def stats(out, y):
    """``mse``, ``r2 = 1 - mse / var(y)``, ``r2_msq = 1 - mse / mean(y^2)`` of fp32 data in ``np.longdouble``, two-pass (the
    mean first), and the two ratios that amplify the error of a single-pass ``var = msq - mean^2``: ``msq / var`` (the
    cancellation) and ``mse / var`` (how much of it reaches ``1 - mse / var``).  A variance of exactly 0 gives ``-inf``."""
    o = np.asarray(torch.as_tensor(out).detach().cpu().numpy(), dtype=np.longdouble).ravel()
    t = np.asarray(torch.as_tensor(y).detach().cpu().numpy(), dtype=np.longdouble).ravel()
    n = np.longdouble(len(t))
    mse = np.square(o - t).sum() / n
    mean = t.sum() / n
    var = np.square(t - mean).sum() / n
    msq = np.square(t).sum() / n
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.longdouble(1) - mse / var if var > 0 else np.longdouble(-np.inf)
        cond_var, cond_mse = (msq / var, mse / var) if var > 0 else (np.longdouble(np.inf), np.longdouble(np.inf))
    return {"mse": mse, "r2": r2, "r2_msq": np.longdouble(1) - mse / msq, "msq_over_var": cond_var, "mse_over_var": cond_mse}


def r2_bar(ref):
    """Relative bar for R^2 of a kernel that forms ``var = msq - mean^2`` in fp64."""
    return TOL * (1.0 + float(ref["msq_over_var"]) * float(ref["mse_over_var"]))


def stats_single_pass(out, y):
    """The kernel's own statements in NumPy fp64: one pass, ``var = msq - mean^2``."""
    o = torch.as_tensor(out).detach().cpu().numpy().astype(np.float64).ravel()
    t = torch.as_tensor(y).detach().cpu().numpy().astype(np.float64).ravel()
    mse, mean, msq = np.square(o - t).mean(), t.mean(), np.square(t).mean()
    return {"mse": mse, "r2": 1.0 - mse / (msq - mean * mean), "r2_msq": 1.0 - mse / msq}


def stats_reference_fp32(out, y):
    """The reference's own formula (DNN_tools.py:144-155) in ``torch.float32`` on the CPU."""
    out, y = torch.as_tensor(out).detach().cpu().float(), torch.as_tensor(y).detach().cpu().float()
    crit = torch.nn.MSELoss()
    loss = crit(out, y)
    return {"mse": float(loss), "r2": float(1.0 - loss / crit(y, torch.mean(y) + torch.zeros_like(y))),
            "r2_msq": float(1.0 - loss / crit(y, torch.zeros_like(y)))}


def stats_data(n, family="training", seed=0):
    """``out, y`` (fp32, CPU).  ``training``: uniform in [-1, 0] as the scaled windows are.  ``offset``: ``y = 100 + 1e-3
    noise`` with the same uniform noise and ``out`` 3e-5 of normal noise off it: ``msq / var`` is 1.2e11, the
    ill-conditioned family.  (Its mean, 99.9995, lies half-way between two fp32 numbers, as a mean usually does; with
    centred noise the mean is 100 to 1e-6, which fp32 holds exactly - a family that flatters the fp32 formula.)"""
    g = _generator("stats", family, n, seed)
    if family == "training":
        return (torch.rand(n, generator=g, dtype=torch.float32) - 1.0, torch.rand(n, generator=g, dtype=torch.float32) - 1.0)
    if family == "offset":
        y = 100.0 + 1e-3 * (torch.rand(n, generator=g, dtype=torch.float32) - 1.0)
        return y + 3e-5 * torch.randn(n, generator=g, dtype=torch.float32), y
    raise ValueError(family)
