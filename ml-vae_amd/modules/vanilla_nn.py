"""VanillaNN on the HIP GEMM: the call surface of speechbrain.lobes.models.VanillaNN that the
HMM_DNN_ALI recipe uses (ref:src/models/HMM_DNN_ALI/model.yaml:39-43): ``dnn_blocks`` times a
Linear(bias=True) to ``dnn_neurons`` plus the activation.  The activation is fused into the GEMM
epilogue, which has LeakyReLU(0.01) and nothing else: any other activation is refused.
"""
from torch import nn

from modules.linear import Linear
from mlvae_hip import ops


class VanillaNN(nn.Module):
    def __init__(self, input_shape, activation=nn.LeakyReLU, dnn_blocks=2, dnn_neurons=512):
        super().__init__()
        act = activation() if isinstance(activation, type) or not isinstance(activation, nn.Module) else activation
        if not isinstance(act, nn.LeakyReLU) or act.negative_slope != 0.01:
            raise ValueError(f"VanillaNN: the fused epilogue is LeakyReLU(0.01), got {act!r}")
        size = int(input_shape[-1])
        self.blocks = nn.ModuleList()
        for _ in range(int(dnn_blocks)):
            self.blocks.append(Linear(size, dnn_neurons, bias=True))
            size = int(dnn_neurons)

    def forward(self, x):
        for lin in self.blocks:
            x = ops.linear(x, lin.w.weight, lin.w.bias, True)
        return x
