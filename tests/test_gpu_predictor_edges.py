"""The native predictor (csrc/saa_predictor.hip) at the edges of its tiles, chunks and LDS, against the same weights
evaluated in fp64.

gemm_nt_kernel computes 64 x 208 tiles of C with K in chunks of 32 (two MFMA groups of 16 k each), split over K as
pick_splits decides; lstm_recurrence_kernel holds 40 * H * (n_p + 1) bytes of LDS per phase and projects the inputs of
encoder layer 1 on the matrix cores in chunks of 32 time steps.  The shapes put M = n_p * n_s and n_s, N = 8H and I, and
K = I and 2H on both sides of those edges, and n_p * H up to the device's LDS per workgroup and one step past it.

The models are not saturated: the input weights of encoder layer 0 and of the decoder are drawn so that the gate
pre-activations are O(1) (with PyTorch's default init thousands of inputs put them several units out, where a lost input
column barely moves the table).  Every shape shows its own sensitivity: the fp64 table moves by at least 10 x the bar when
one boundary column of the window's history is dropped."""
import math
import warnings

import pytest
import torch

from predictor_double import TOL, fp64_table
from synchronization_avoiding_algorithms_amd import _lib
from synchronization_avoiding_algorithms_amd import predictor as pr

pytestmark = pytest.mark.gpu

KBM, KBN, KKC = 64, 208, 32  # gemm_nt_kernel: rows and columns of a tile of C, length of a K chunk


def _cdiv(a, b):
    return -(-a // b)


def pick_splits(M, N, K, n_cu):
    """pick_splits of csrc/saa_predictor.hip restated: (number of K slices, slice length; the last slice may be shorter)."""
    tiles = _cdiv(M, KBM) * _cdiv(N, KBN)
    best, splits, kps = -1e30, 1, _cdiv(K, KKC) * KKC
    for s in range(1, max(1, K // 128) + 1):
        k = _cdiv(_cdiv(K, s), KKC) * KKC
        s_eff = _cdiv(K, k)
        wgs, slots = tiles * s_eff, 2 * n_cu
        score = wgs / (_cdiv(wgs, slots) * slots) - 0.01 * s_eff
        if score > best:
            best, splits, kps = score, s_eff, k
    return splits, kps


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lds_limit():
    """LDS one workgroup may hold, as the device reports it (what saa_predictor_create compares against)."""
    return torch.cuda.get_device_properties(0).shared_memory_per_block


def _lds_bytes(H, n_p):
    return 40 * H * (n_p + 1)  # lstm_recurrence_kernel: gates, h, the layer-0 outputs and the projections, fp32


def _first_n_past_beyond_the_lds(H):
    return _lds_limit() // (40 * H)


# n_p = None: the largest n_p whose recurrence fits the device's LDS (80 at H = 50 and 31 at H = 128 for 160 KiB)
SHAPES = [
    # I    H    n_p   n_f n_s
    (31,   26,  3,    3,  21),  # M1 = 63; N = 8H = 208, one column tile; K = 31, one short chunk
    (32,   27,  4,    2,  16),  # M1 = 64; N = 216, one column over; K = 32
    (33,   8,   5,    5,  13),  # M1 = 65; K = 33: the second chunk holds k = 32 alone; output K = 2H = 16, one MFMA group
    (127,  17,  8,    4,  16),  # M1 = 128; K = 127; output K = 34: a second chunk with two k
    (128,  52,  3,    3,  43),  # M1 = 129; N = 416, two column tiles; K = 128
    (129,  50,  33,   2,  4),   # register kernel: layer 1 projected in two 32-step chunks (68 000 B LDS); K = 129
    (208,  50,  None, 2,  3),   # register kernel at the LDS limit; output N = 208
    (209,  64,  40,   3,  2),   # generic kernel above 64 KiB (104 960 B); output N = 209
    (416,  128, None, 2,  2),   # the widest model at the LDS limit; N = 1024; output N = 416
    (417,  17,  2,    1,  64),  # n_s = 64: the decoder's GEMM one full row tile; a single decoder step; output N = 417
    (4133, 52,  2,    3,  65),  # K above 4096: split-K with a shorter last slice; n_s = 65
    (1000, 128, 3,    2,  65),  # split-K in both input GEMMs (ten tiles in the decoder's)
]


def _resolve(shape):
    I, H, n_p, n_f, n_s = shape
    return I, H, (_first_n_past_beyond_the_lds(H) - 1 if n_p is None else n_p), n_f, n_s


def _case(I, H, n_p, n_s):
    """A model whose input weights give O(1) gate pre-activations, and a random-walk history of n_p * n_s + 7 rows."""
    torch.manual_seed(1000 * H + I)
    model = pr.LSTM_encoder_decoder(I, H)
    # the scaled inputs lie in [-1, 0] with an rms of about 0.5: U(-a, a) with a = 2 sqrt(3 / I) gives a sum of I terms a
    # standard deviation of about 1 (the default init, a = 1 / sqrt(H), gives sqrt(I / 3H) / 2: 4 at I = 9126, H = 50)
    a = 2.0 * math.sqrt(3.0 / I)
    with torch.no_grad():
        for w in (model.encoder.lstm_encoder.weight_ih_l0, model.encoder.lstm_encoder.weight_ih_l0_reverse,
                  model.decoder.lstm_decoder.weight_ih_l0):
            w.uniform_(-a, a)
    model = model.cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(I + H)
    hist = torch.cumsum(torch.randn(n_p * n_s + 7, I, generator=gen, device="cuda", dtype=torch.float64) * 1e-4, 0)
    smax, smin = float(hist.max()) * 1.1, float(hist.min()) * 1.1
    return model, hist, smax, smin


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "I{}-H{}-np{}-nf{}-ns{}".format(*[v or "lds" for v in s]))
def test_edge_shapes_against_the_fp64_evaluation(shape):
    I, H, n_p, n_f, n_s = _resolve(shape)
    M1 = n_p * n_s
    model, hist, smax, smin = _case(I, H, n_p, n_s)
    n = hist.shape[0] - 3
    nat = pr.NativePredictor(model, n_p, n_f, n_s)
    got = nat.predict(n, hist, smax, smin)
    ref = fp64_table(model, n, n_p, n_f, n_s, hist, smax, smin)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / scale
    # not saturated: encoder layer 0's input projections of the window
    X = pr.scale_forward(hist[n - M1:n], smax, smin)
    pre_std = float((X @ model.encoder.lstm_encoder.weight_ih_l0.detach().double().t()).std())
    # the mutation: one boundary column of K scaled to 0 in every row of the window - what a kernel that loses it computes
    S1, kps1 = pick_splits(M1, 8 * H, I, _n_cu())
    k = (S1 - 1) * kps1 - 1 if S1 > 1 else min(KKC, I - 1)
    mutated = hist.clone()
    mutated[n - M1:n, k] = smax
    moved = float((fp64_table(model, n, n_p, n_f, n_s, mutated, smax, smin) - ref).abs().max()) / scale
    print(f"I={I} H={H} n_p={n_p} n_f={n_f} n_s={n_s}: LDS {_lds_bytes(H, n_p)} B, S1={S1}, error/range {err:.2e}, "
          f"pre-activation std {pre_std:.2f}, column {k} dropped moves {moved:.2e}")
    assert err <= TOL, (shape, err)
    assert moved >= 10 * TOL, (shape, k, moved)
    assert 0.3 <= pre_std <= 3.0, (shape, pre_std)
    assert torch.equal(got, nat.predict(n, hist, smax, smin))  # fixed summation orders
    assert torch.equal(got, got.float().double())  # fp32 values widened
    nat.close()


def test_the_shapes_cover_every_split_case():
    """With this device's CU count the sweep has a shape without split-K, one with a shorter last K slice and one with
    the decoder's GEMM split too (which one is not pinned: pick_splits may change)."""
    n_cu, cases = _n_cu(), []
    for shape in SHAPES:
        I, H, n_p, n_f, n_s = _resolve(shape)
        S1, kps1 = pick_splits(n_p * n_s, 8 * H, I, n_cu)
        S2, _ = pick_splits(n_s, 8 * H, I, n_cu)
        cases.append((S1, I - (S1 - 1) * kps1 < kps1, S2))
    assert any(S1 == 1 for S1, _, _ in cases), cases
    assert any(S1 > 1 and short for S1, short, _ in cases), cases
    assert any(S2 > 1 for _, _, S2 in cases), cases


@pytest.mark.parametrize("H", [50, 128])
def test_the_first_n_past_beyond_the_lds_is_refused_and_device_predictor_falls_back(H):
    n_p, I, n_f, n_s = _first_n_past_beyond_the_lds(H), 24, 2, 3
    assert _lds_bytes(H, n_p) > _lds_limit() >= _lds_bytes(H, n_p - 1)
    model, hist, smax, smin = _case(I, H, n_p, n_s)
    with pytest.raises(_lib.SaaError, match="LDS"):
        pr.NativePredictor(model, n_p, n_f, n_s)
    n = hist.shape[0] - 3
    dev = pr.DevicePredictor(model, n_p, n_f, n_s, smax, smin, graph=False)
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        tables = [dev(n, hist).clone() for _ in range(2)]
        want = pr.predict_table(model, n, n_p, n_f, n_s, hist, smax, smin)
    refused = [w for w in caught if "native predictor refused" in str(w.message)]
    assert len(refused) == 1 and "LDS" in str(refused[0].message), [str(w.message) for w in caught]
    assert dev.backend.startswith("PyTorch-ROCm")
    for t in tables:
        assert float((t - want).abs().max()) <= 1e-4 * float(want.abs().max())


def test_history_stride_at_the_32_bit_limit():
    """The largest row stride saa_predictor_predict takes (63 rows of it plus a row's inputs below 2 GiB: the GEMM forms
    a tile's row offsets in 32 bits) with a window of 68 rows, so that the first row tile spans all 64 rows (2.4 GB of
    device memory, NaN wherever the history is not); one more is refused."""
    I, H, n_p, n_f, n_s = 24, 50, 2, 2, 34
    M1 = n_p * n_s
    ld = ((1 << 31) - 1 - 8 * I) // (63 * 8)
    assert 63 * ld * 8 + I * 8 < 1 << 31 <= 63 * (ld + 1) * 8 + I * 8
    model, small, smax, smin = _case(I, H, n_p, n_s)
    rows = M1 + 2
    buf = torch.full(((rows - 1) * ld + I,), float("nan"), dtype=torch.float64, device="cuda")
    hist = buf.as_strided((rows, I), (ld, 1))
    hist.copy_(small[:rows])
    nat = pr.NativePredictor(model, n_p, n_f, n_s)
    for n in (M1, rows):
        got = nat.predict(n, hist, smax, smin)
        assert torch.isfinite(got).all() and torch.equal(got, nat.predict(n, hist.contiguous(), smax, smin)), n
    with pytest.raises(_lib.SaaError, match="stride"):
        nat.predict(M1, buf.as_strided((M1, I), (ld + 1, 1)), smax, smin)
    nat.close()
    del buf, hist
    torch.cuda.empty_cache()
