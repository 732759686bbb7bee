"""The bar of tests/test_gpu_training_edges.py proved on the CPU, before any GPU sees it (tests/training_double.py):

* ``env <= 1e-5`` on every recurrence and cell case, so that ``8 env`` is a statement about round-off;
* a wrong reference shows: zeroing the last column of ``W``, or giving the last processed step its neighbour's ``pre``
  row, moves ``H`` by at least 100 bars;
* the fp32 restatement of the kernel's own form (``tanh`` on the tanh gate, ``1 / (1 + exp(-x))``) stays within ``2 env``
  on every field, finite in the saturated families;
* the bar has teeth: the form ``lstm_rec_forward_kernel`` had before, ``tanh v = 2 s(2v) - 1``, FAILS it in ``H`` on the
  small-signal families and passes on all others;
* the longdouble two-pass statistics agree with the single-pass fp64 statements of the kernel to 1e-12 where ``y`` is
  well conditioned, and the R^2 bar covers the single-pass form where it is not."""
import numpy as np
import pytest
import torch

import training_double as td

REC_CASES = [(f, w, r) for f in td.REC_FAMILIES for w in td.WIDTHS for r in (False, True)]
STATS_N = (63, 64, 65, 1023, 1024, 1025, 4096, 4097, 128 * 4096 - 1, 128 * 4096, 128 * 4096 + 1, 3 * 128 * 4096 + 5)


def _ratio(e, env):
    return e / env if env > 0 else (0.0 if e == 0 else float("inf"))


@pytest.mark.parametrize("family,width,reverse", REC_CASES)
def test_recurrence_bar_is_meaningful_and_can_fail(family, width, reverse):
    inp = td.rec_inputs(family, width, reverse)
    for state, (has_h0, _) in td.STATES.items():
        label = (family, width, reverse, state)
        env, ref = td.rec_env(family, width, reverse, state), td.rec_reference(family, width, reverse, state)
        assert set(env) == set(ref) and max(env.values()) <= td.ENV_MAX, (label, env)
        bar = td.KERNEL_FACTOR * env["H"]
        # a single step from a zero h does not read W, and has no neighbour
        moves = {m: td.err(td.rec_outputs(inp, state, mutate=m)["H"], ref["H"])
                 for m in ("w_column", "pre_neighbour") if inp["T"] >= 2 or (m == "w_column" and has_h0)}
        assert all(v >= td.SENSITIVITY * bar for v in moves.values()), (label, moves, bar)
        own = td.errors(td.rec_outputs(inp, state, torch.float32, "kernel"), ref)
        assert all(own[k] <= td.STABLE_FACTOR * env[k] for k in env), (label, own, env)
        old = td.errors(td.rec_outputs(inp, state, torch.float32, "two_sigmoid"), ref)
        print(label, "env(H) %.1e" % env["H"], "own/env %.2f" % max(_ratio(own[k], env[k]) for k in env),
              "two_sigmoid/env: H %.1f, worst %.1f" % (_ratio(old["H"], env["H"]), max(_ratio(old[k], env[k]) for k in env)),
              "moved/bar", {m: "%.0f" % (v / bar) for m, v in moves.items()})
        if family in td.SMALL_SIGNAL:
            assert old["H"] > td.KERNEL_FACTOR * env["H"] and old["dW"] > td.KERNEL_FACTOR * env["dW"], (label, old, env)
        else:
            assert all(old[k] <= td.KERNEL_FACTOR * env[k] for k in env), (label, old, env)


def test_saturated_families_are_saturated_and_small_ones_small():
    """The families are what their names say: past the overflow of fp32 ``exp`` in one, a tanh gate below 1e-2 in the other
    (where ``2 s(2v) - 1`` has lost two of its seven digits and more)."""
    assert float(td.rec_inputs("saturated100", 100, False)["pre"].abs().max()) > 88.73
    assert float(td.rec_inputs("saturated", 50, False)["pre"].abs().max()) > 88.73 / 2      # 2v overflows in the old form
    for family in td.SMALL_SIGNAL:
        for width in td.WIDTHS:
            assert float(td.rec_reference(family, width, False, "both")["H"].abs().max()) < 1e-2


@pytest.mark.parametrize("B,D,scale", td.CELL_CASES)
def test_cell_env_is_round_off(B, D, scale):
    env = td.cell_env(B, D, scale)
    print((B, D, scale), {k: "%.1e" % v for k, v in env.items()})
    assert set(env) == set(td.CELL_FIELDS) and 0.0 < min(env.values()) and max(env.values()) <= td.ENV_MAX, env


def test_statistics_two_pass_against_single_pass():
    for n in STATS_N:
        out, y = td.stats_data(n)
        ref, one = td.stats(out, y), td.stats_single_pass(out, y)
        assert float(ref["msq_over_var"]) < 8.0 and float(ref["mse_over_var"]) < 4.0, (n, ref)  # well conditioned
        for k in ("mse", "r2", "r2_msq"):
            assert abs(one[k] - float(ref[k])) <= td.TOL * abs(float(ref[k])), (n, k, one[k], ref[k])
    ref = td.stats(*td.stats_data(1))
    assert ref["r2"] == -np.inf and np.isfinite(float(ref["mse"])) and ref["mse"] > 0


def test_r2_bar_covers_the_single_pass_form_where_y_is_ill_conditioned():
    """``y = 100 + 1e-3 noise``: ``msq / var`` is 1e11, the single-pass fp64 variance keeps five digits, and the R^2 bar
    ``1e-12 (1 + msq/var mse/var)`` is what that costs; the reference's own fp32 formula is further off than fp64."""
    out, y = td.stats_data(200 * 3042, "offset")
    ref, one, f32 = td.stats(out, y), td.stats_single_pass(out, y), td.stats_reference_fp32(out, y)
    assert float(ref["msq_over_var"]) > 1e9
    e64, e32 = abs(one["r2"] - float(ref["r2"])), abs(f32["r2"] - float(ref["r2"]))
    print("R^2 %.6f: single-pass fp64 off by %.1e, the fp32 formula by %.1e, bar %.1e" % (float(ref["r2"]), e64, e32,
                                                                                      td.r2_bar(ref) * abs(float(ref["r2"]))))
    assert e64 <= td.r2_bar(ref) * abs(float(ref["r2"])) and e64 <= e32


def test_row_count_families_straddle_the_weight_gradient_threshold():
    from synchronization_avoiding_algorithms_amd import training as tr

    rows = {f: td.REC_FAMILIES[f][0] * td.REC_FAMILIES[f][1] for f in ("B25", "B26", "B300")}
    assert rows["B25"] <= tr._DW_ONE_PRODUCT_ROWS < rows["B26"] < rows["B300"]
