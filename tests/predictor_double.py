"""The predictor model evaluated in fp64 - what the native predictor kernels (csrc/saa_predictor.hip) are measured
against - and the bar they are held to.  Shared by test_gpu_predictor.py and test_gpu_predictor_edges.py."""
import copy

import numpy as np
import torch

from synchronization_avoiding_algorithms_amd import predictor as pr

# fp32 round-off carried through 2 x n_p + n_f recurrent steps: the kernels' largest difference from the fp64 evaluation,
# as a share of the table's range
TOL = 2e-5


def fp64_table(model, n, n_p, n_f, n_s, hist, smax, smin):
    """The same model evaluated in fp64 on the history's device (weights widened, the scaled history not rounded to
    fp32)."""
    m64 = copy.deepcopy(model).double()
    past, fut = pr._phase_indices(n, n_p, n_f, n_s)
    with torch.no_grad():
        X = pr.scale_forward(hist[torch.as_tensor(np.stack(past), device=hist.device)], smax, smin)
        Y = pr.scale_it_back(pr.model_predict(hist.device, m64, X, n_f), smax, smin)
    table = torch.zeros((n_s * n_f, hist.shape[1]), dtype=torch.float64, device=hist.device)
    table[torch.as_tensor(np.stack(fut), device=hist.device).reshape(-1)] = Y.reshape(-1, hist.shape[1])
    return table
