"""Linear on the HIP GEMM: the call surface of speechbrain.nnet.linear.Linear that the
HMM_DNN_ALI recipe uses (ref:src/models/HMM_DNN_ALI/model.yaml:45-48): ``w`` is an nn.Linear, so
state_dict keys are ``w.weight`` / ``w.bias`` as SpeechBrain's.
"""
from torch import nn

from mlvae_hip import ops


class Linear(nn.Module):
    def __init__(self, input_size, n_neurons, bias=True):
        super().__init__()
        self.w = nn.Linear(int(input_size), int(n_neurons), bias=bias)

    def forward(self, x):
        return ops.linear(x, self.w.weight, self.w.bias)
