"""LSTM training counterpart of Model_training.py: windowing/scaling equal the inference-side constants,
the loss goes down, and the saved state_dict feeds call_model / the predictor (CPU, tiny)."""
import os

import numpy as np
import torch

from synchronization_avoiding_algorithms_amd import drivers, predictor as pr, results_io as rio, training as tr


def _fake_shared_trajectory(n_in=6, n_steps=1200):
    t = np.arange(n_steps)[None, :]
    j = np.arange(n_in)[:, None]
    return 1e-2 * np.sin(0.01 * t + 0.5 * j) * (1 + 0.05 * j)


def test_windowing_and_scaling_match_inference_side():
    traj = _fake_shared_trajectory()
    X, Y = tr.windowed_dataset(traj, 10, 4, 3, 0.5)
    assert X.shape == (54, 4, 6) and Y.shape == (54, 3, 6) and X.dtype == torch.float32
    # window k: inputs = filtered samples k..k+3, targets k+4..k+6 (DNN_tools.py:303-307)
    filt = traj.T[:600][::10].astype(np.float32)
    assert np.array_equal(X[5].numpy(), filt[5:9]) and np.array_equal(Y[5].numpy(), filt[9:12])
    Xs, Ys, smax, smin = tr.scale_to_zero_one(X, Y)
    assert (smax, smin) == pr.scaling_constants(traj, 10, 4, 3, 0.5)
    assert float(Xs.max()) <= 0.0 and float(min(Xs.min(), Ys.min())) == -1.0


def test_training_reduces_loss_and_writes_reference_layout(tmp_path):
    out = str(tmp_path)
    traj = _fake_shared_trajectory()
    rio.save_int_list(os.path.join(out, drivers.PATHS["shared"].format(r=0)), [3, 9])
    rio.save_displacement(os.path.join(out, drivers.PATHS["shared_traj"].format(r=0)), traj, compress=False)
    path, train_loss, test_loss = tr.train_rank_model(out, 0, device="cpu", hidden_size=8, filter_size=10, n_past=4,
                                                      n_future=3, num_epochs=40, learning_rate=5e-3, seed=0)
    assert path.endswith("Distributed_save/Rank-0/nB-10-nH-8-Lr-0.005-filter=10/model.pth")
    assert train_loss[-1] < 0.2 * train_loss[0] and np.isfinite(test_loss).all()
    model = pr.call_model("cpu", 10, 6, 8, path)
    hist = torch.from_numpy(traj.T.copy())
    smax, smin = pr.scaling_constants(traj, 10, 4, 3, 0.5)
    table = pr.predict_table(model, 400, 4, 3, 10, hist, smax, smin)
    assert table.shape == (30, 6) and torch.isfinite(table).all()
    # a (briefly) trained model tracks the smooth signal far better than the mean would
    err = (table - hist[400:430]).abs().max().item()
    assert err < 0.5 * (smax - smin)


import pytest  # noqa: E402


@pytest.mark.gpu
def test_graph_captured_training_step_matches_eager_training(tmp_path):
    """On the GPU the optimiser step is replayed as a HIP graph (GraphedTrainStep): same seeds, same batches, same
    learning-rate schedule as eager training -> the same losses up to fp32 run-to-run noise."""
    traj = _fake_shared_trajectory(n_in=12, n_steps=4000)
    losses, paths = [], []
    for mode in (0, 1):
        out = str(tmp_path / f"graph{mode}")
        rio.save_int_list(os.path.join(out, drivers.PATHS["shared"].format(r=0)), [3, 9, 11, 17])
        rio.save_displacement(os.path.join(out, drivers.PATHS["shared_traj"].format(r=0)), traj, compress=False)
        path, train_loss, test_loss = tr.train_rank_model(out, 0, device="cuda", hidden_size=8, filter_size=10, n_past=4,
                                                          n_future=3, num_epochs=12, learning_rate=5e-3, seed=0,
                                                          graph=bool(mode))
        losses.append((np.array(train_loss), np.array(test_loss)))
        paths.append(path)
    (tl0, vl0), (tl1, vl1) = losses
    assert tl1[-1] < 0.5 * tl1[0]
    assert np.allclose(tl1, tl0, rtol=2e-2) and np.allclose(vl1, vl0, rtol=2e-2)
    a, b = torch.load(paths[0], weights_only=True), torch.load(paths[1], weights_only=True)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.allclose(a[k], b[k], rtol=0, atol=5e-3), k


def test_training_from_a_history_tensor_matches_the_file_path(tmp_path):
    """``windows_from_history`` / ``train_on_history`` (what bench.py's sync-avoiding leg uses: the shared-dof history a
    synchronised run left in memory, ``d_sol_shared`` layout) give the windows, scaling constants and - with the same
    seed - the model of the file-based ``train_rank_model`` (Shared_extraction.py layout, the transpose)."""
    traj = _fake_shared_trajectory(n_in=6, n_steps=900)          # (in, steps) as Shared_extraction.py stores it
    hist = torch.from_numpy(traj.T.copy())                        # (steps, in) as Online_predictor.py:260 fills it
    X, Y = tr.windowed_dataset(traj, 10, 4, 3, 1.0)
    Xh, Yh = tr.windows_from_history(hist, 10, 4, 3, 1.0)
    assert torch.equal(X, Xh) and torch.equal(Y, Yh)
    model, smax, smin, tl, vl = tr.train_on_history(hist, 10, 4, 3, cut_off=1.0, seed=3, hidden_size=8, num_epochs=5,
                                                    learning_rate=5e-3)
    assert (smax, smin) == pr.scaling_constants(traj, 10, 4, 3, 1.0)
    assert len(tl) == len(vl) == 5 and tl[-1] < tl[0] and not model.training
    out = str(tmp_path)
    rio.save_int_list(os.path.join(out, drivers.PATHS["shared"].format(r=0)), [3, 9])
    rio.save_displacement(os.path.join(out, drivers.PATHS["shared_traj"].format(r=0)), traj, compress=False)
    path, tl2, _ = tr.train_rank_model(out, 0, device="cpu", hidden_size=8, filter_size=10, n_past=4, n_future=3,
                                       cut_off=1.0, num_epochs=5, learning_rate=5e-3, seed=3)
    assert np.allclose(tl, tl2, rtol=1e-6)
    saved = torch.load(path, weights_only=True)
    for k, v in model.state_dict().items():
        assert torch.allclose(v, saved[k], atol=1e-6), k
    # the time bound ends training early
    _, _, _, tl3, _ = tr.train_on_history(hist, 10, 4, 3, seed=3, hidden_size=8, num_epochs=10000, max_seconds=0.5)
    assert 1 <= len(tl3) < 10000


def test_folded_decoding_is_the_same_function_forward_and_backward():
    """``training._decode_folded`` (what the GPU path trains through: the decoder's feedback folded into its recurrent
    matrix) against the literal recursion of DNN_tools.py:119-127, on the CPU where both run: outputs and the gradients
    with respect to every parameter agree to fp32 round-off."""
    import torch

    from synchronization_avoiding_algorithms_amd import predictor as pr
    from synchronization_avoiding_algorithms_amd import training as tr

    torch.manual_seed(0)
    model = pr.LSTM_encoder_decoder(30, 8)
    X = torch.randn(5, 6, 30) * 0.3
    folded = tr._decode_folded(model, X, 4)
    h, c = model.encoder(X)
    inp, outs = X[:, -1, :], []
    for _ in range(4):
        inp, h, c = model.decoder(inp, h, c)
        outs.append(inp)
    literal = torch.stack(outs, 1)
    assert folded.shape == literal.shape and float((folded - literal).abs().max()) < 5e-7
    ga = torch.autograd.grad(folded.square().mean(), list(model.parameters()))
    gb = torch.autograd.grad(literal.square().mean(), list(model.parameters()))
    scale = max(float(g.abs().max()) for g in gb)
    assert max(float((a - b).abs().max()) for a, b in zip(ga, gb)) < 1e-6 * scale
    # the CPU path itself keeps the literal form (the reference-pinned tolerances of test_training_golden.py are its)
    assert torch.equal(tr._decode(model, X, 4), literal)


@pytest.mark.gpu
def test_fused_cell_kernels_forward_and_backward_on_gpu():
    """``saa_lstm_cell_forward`` / ``_backward`` (the pointwise part of an LSTM step in the training pass) against the
    elementwise PyTorch formulation and its autograd gradients, incl. a step whose cell output has no gradient."""
    import torch

    from synchronization_avoiding_algorithms_amd import training as tr

    torch.manual_seed(0)
    # 255, 256, 257 elements: a last workgroup of 255 threads, none ragged, one thread alone; then more than 2^20
    for B, D in ((10, 100), (3, 7), (1, 1), (5, 51), (2, 128), (1, 257), (1025, 1024)):
        gates = torch.randn(B, 4 * D, device="cuda", requires_grad=True)
        c0 = torch.randn(B, D, device="cuda", requires_grad=True)
        wh, wc = torch.randn(B, D, device="cuda"), torch.randn(B, D, device="cuda")
        h, c = tr._FusedCell.apply(gates, c0)
        gi, gf, gg, go = gates.chunk(4, dim=1)
        c_ref = torch.sigmoid(gf) * c0 + torch.sigmoid(gi) * torch.tanh(gg)
        h_ref = torch.sigmoid(go) * torch.tanh(c_ref)
        assert torch.allclose(h, h_ref, atol=2e-6) and torch.allclose(c, c_ref, atol=2e-6)
        for use_c in (True, False):
            loss = (h * wh).sum() + ((c * wc).sum() if use_c else 0.0)
            ref = (h_ref * wh).sum() + ((c_ref * wc).sum() if use_c else 0.0)
            ga = torch.autograd.grad(loss, (gates, c0), retain_graph=True)
            gb = torch.autograd.grad(ref, (gates, c0), retain_graph=True)
            assert all(torch.allclose(a, b, atol=5e-6) for a, b in zip(ga, gb)), (B, D, use_c)


@pytest.mark.gpu
def test_folded_fused_decoding_matches_the_literal_recursion_on_gpu():
    import torch

    from synchronization_avoiding_algorithms_amd import predictor as pr
    from synchronization_avoiding_algorithms_amd import training as tr

    torch.manual_seed(0)
    model = pr.LSTM_encoder_decoder(45, 50).cuda()
    X = torch.randn(10, 20, 45, device="cuda") * 0.3
    folded = tr._decode(model, X, 20)  # GPU default: folded feedback, fused cell
    h, c = model.encoder(X)
    inp, outs = X[:, -1, :], []
    for _ in range(20):
        inp, h, c = model.decoder(inp, h, c)
        outs.append(inp)
    literal = torch.stack(outs, 1)
    assert float((folded - literal).detach().abs().max()) < 5e-6
    ga = torch.autograd.grad(folded.square().mean(), list(model.parameters()))
    gb = torch.autograd.grad(literal.square().mean(), list(model.parameters()))
    scale = max(float(g.abs().max()) for g in gb)
    assert max(float((a - b).abs().max()) for a, b in zip(ga, gb)) < 2e-5 * scale


def test_batched_validation_equals_the_batch_loop():
    """One forward pass over all validation windows + segment sums == the reference's loop over the validation batches
    (model_test, DNN_tools.py:170-207), incl. a last batch of one window."""
    import torch
    import torch.nn as nn

    from synchronization_avoiding_algorithms_amd import predictor as pr
    from synchronization_avoiding_algorithms_amd import training as tr

    torch.manual_seed(0)
    model = pr.LSTM_encoder_decoder(30, 8)
    X, Y = torch.rand(41, 6, 30) - 1.0, torch.rand(41, 4, 30) - 1.0
    vb = tr._batches(X, Y, 10, False)
    crit = nn.MSELoss()
    want = tr.model_test("cpu", model, vb, crit, 4)
    got = tr.BatchedValidation(model, crit, vb, 4, torch.device("cpu")).run()
    assert all(abs(a - b) <= 1e-6 * max(1.0, abs(b)) for a, b in zip(got, want)), (got, want)


@pytest.mark.gpu
def test_train_stats_kernel_against_the_formulas():
    """``saa_train_stats``: mse, 1 - mse/var(y), 1 - mse/mean(y^2) added to running sums (DNN_tools.py:144-155).  A single
    target value (variance 0, R^2 = -inf) has sums of its own: added to the others it would turn their R^2 into -inf too,
    whatever the kernel's variance is.  R^2 is held to ``1e-12 (1 + msq/var mse/var)`` (tests/training_double.py)."""
    import torch

    import training_double as td
    from synchronization_avoiding_algorithms_amd import _lib

    torch.manual_seed(0)
    lib = _lib.load()
    scratch = torch.zeros(3, dtype=torch.float64, device="cuda")

    def add(sums, n):
        out, y = torch.rand(n, device="cuda") - 1.0, torch.rand(n, device="cuda") - 1.0 if n > 1 else torch.full((1,), -0.3, device="cuda")
        _lib.check(lib.saa_train_stats(0, n, out.data_ptr(), y.data_ptr(), scratch.data_ptr(), sums.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
        o, t = out.double().cpu(), y.double().cpu()
        mse = (o - t).square().mean()
        r2 = 1 - mse / (t - t.mean()).square().mean() if n > 1 else torch.tensor(float("-inf"), dtype=torch.float64)
        ref = td.stats(out, y)
        return torch.stack([mse, r2, 1 - mse / t.square().mean()]), (td.r2_bar(ref) * abs(float(ref["r2"])) if n > 1 else 0.0)

    sums, want, bar = torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64), 0.0
    for n in (63, 200 * 3042, 1 << 20):
        w, b = add(sums, n)
        want, bar = want + w, bar + b
    got = sums.cpu()
    assert torch.allclose(got[[0, 2]], want[[0, 2]], rtol=1e-12) and float(scratch.abs().sum()) == 0.0
    assert abs(float(got[1] - want[1])) <= bar, (got[1], want[1], bar)
    single = torch.zeros(3, dtype=torch.float64, device="cuda")
    want, _ = add(single, 1)
    got = single.cpu()
    assert torch.allclose(got[[0, 2]], want[[0, 2]], rtol=1e-12) and float(scratch.abs().sum()) == 0.0
    assert got[1] == want[1] and torch.isinf(got[1]) and got[1] < 0  # a single target value: variance 0


@pytest.mark.gpu
@pytest.mark.parametrize("width", [50, 100])
@pytest.mark.parametrize("reverse", [False, True])
def test_whole_recurrence_kernels_against_step_by_step_autograd(width, reverse):
    """``saa_lstm_recurrence_forward`` / ``_backward`` behind ``training._Recurrence``: every h_t, the final c and the
    gradients with respect to the input projections, the recurrent matrix and the initial states against the same
    recurrence written step by step in PyTorch ops, in fp32 and in fp64.  T = 1 and 2 are where the kernels' one step
    ahead requests clamp (the forward's next projection, the backward's fetch of the step before); B = 300 is a grid of
    300 workgroups."""
    import torch

    from synchronization_avoiding_algorithms_amd import training as tr

    def step_by_step(pre, W, h, c, T):
        seq = [None] * T
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            gi, gf, gg, go = (pre[:, t, :] + h @ W.t()).chunk(4, dim=1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            h = torch.sigmoid(go) * torch.tanh(c)
            seq[t] = h
        return torch.stack(seq, dim=1), c

    torch.manual_seed(width + int(reverse))
    H = width
    for B, T in ((7, 9), (1, 1), (1, 2), (300, 20)):
        pre = (torch.randn(B, T, 4 * H, device="cuda") * 0.5).requires_grad_()
        W = (torch.randn(4 * H, H, device="cuda") * 0.2).requires_grad_()
        h0 = (torch.randn(B, H, device="cuda") * 0.3).requires_grad_()
        c0 = (torch.randn(B, H, device="cuda") * 0.3).requires_grad_()
        wh, wc = torch.randn(B, T, H, device="cuda"), torch.randn(B, H, device="cuda")
        # the same leaves widened: the fp64 reference
        pre64, W64, h064, c064 = (x.detach().double().requires_grad_() for x in (pre, W, h0, c0))
        for with_state in (True, False):
            Hall, cT = tr._Recurrence.apply(pre, h0 if with_state else None, c0 if with_state else None, W, reverse)
            wrt = (pre, W, h0, c0) if with_state else (pre, W)
            ga = torch.autograd.grad((Hall * wh).sum() + (cT * wc).sum(), wrt)
            for dt, leaves in ((torch.float32, (pre, W, h0, c0)), (torch.float64, (pre64, W64, h064, c064))):
                p, w, hs, cs = leaves
                h = hs if with_state else torch.zeros(B, H, device="cuda", dtype=dt)
                c = cs if with_state else torch.zeros(B, H, device="cuda", dtype=dt)
                ref, c = step_by_step(p, w, h, c, T)
                case = (B, T, width, reverse, with_state, dt)
                assert float((Hall.double() - ref.double()).detach().abs().max()) < 3e-6, case
                assert float((cT.double() - c.double()).detach().abs().max()) < 3e-6, case
                gb = torch.autograd.grad((ref * wh.to(dt)).sum() + (c * wc.to(dt)).sum(), (p, w, hs, cs) if with_state else (p, w))
                for a, b in zip(ga, gb):
                    assert float((a.double() - b.double()).abs().max()) < 2e-5 * max(1.0, float(b.abs().max())), case
