"""CRDNN on the HIP stack: the keyword surface of speechbrain.lobes.models.CRDNN.CRDNN that the
CRDNN_CTC recipes' yaml passes (ref:src/models/CRDNN_CTC/model.yaml:23-35), built from what this
project has -- ``rnn``: modules.lstm.LSTM (``rnn_layers`` layers of ``rnn_neurons`` units,
bidirectional or not, inter-layer dropout, the persistent HIP recurrence), then ``dnn``:
``dnn_blocks`` times a Linear(bias=True) to ``dnn_neurons`` with LeakyReLU(0.01) fused into the
GEMM epilogue.

``CRDNN`` itself keeps to the recurrent and the DNN part: ``cnn_blocks > 0`` and
``time_pooling=True`` raise NotImplementedError there, and ``cnn_channels`` / ``cnn_kernelsize``
are accepted and unused.  The lobe's convolutional front end lives beside it:

``CNNFront``: ``cnn_blocks`` times (conv_1, norm_1, LeakyReLU, conv_2, norm_2, LeakyReLU,
frequency max-pool 2, Dropout2d), then the optional time max-pool 2 -- Conv2d 3x3 with reflect
"same" padding (SpeechBrain's Conv2d default), LayerNorm over (F, C), on the HIP kernels of
csrc/conv2d.hip (ops.conv2d_3x3, ops.layer_norm_fc_act, ops.time_pool) over channels-last
[B, T, F, C]; the output is [B, T', F_out * C_last], F-major / C-minor.  The Dropout2d draw is one
per (utterance, pooled frequency bin), shared by all frames and channels (the lobe's Dropout2d moves
time last and hands torch.nn.Dropout2d a [B, F', C, T] tensor).  ``ConvCRDNN``: the CRDNN keyword
surface, CNNFront followed by CRDNN.

Out of scope, stated rather than approximated: ``using_2d_pooling``, ``projection_dim``,
``use_rnnp``, the lobe's LiGRU (the recurrent layer here is an LSTM), the BatchNorm and the dropout
inside its DNN blocks; only ``cnn_kernelsize`` (3, 3).  As with every other SpeechBrain lobe in
this project, parity with the lobe is unpinned."""
import torch
from torch import nn

from modules.linear import Linear
from modules.lstm import LSTM
from mlvae_hip import ops


class CRDNN(nn.Module):
    def __init__(self, input_size, activation=nn.LeakyReLU, dropout=0.15, cnn_blocks=0,
                 cnn_channels=(128, 256), cnn_kernelsize=(3, 3), time_pooling=False, rnn_layers=4,
                 rnn_neurons=512, rnn_bidirectional=True, dnn_blocks=2, dnn_neurons=512):
        super().__init__()
        if int(cnn_blocks) > 0 or time_pooling:
            raise NotImplementedError(
                f"CRDNN: cnn_blocks = {cnn_blocks}, time_pooling = {time_pooling}: this build has the "
                "recurrent and the DNN part only (cnn_blocks: 0, time_pooling: False); the SpeechBrain "
                "lobe's Conv2d / LayerNorm / pooling front is not reproduced")
        act = activation() if isinstance(activation, type) or not isinstance(activation, nn.Module) else activation
        if not isinstance(act, nn.LeakyReLU) or act.negative_slope != 0.01:
            raise ValueError(f"CRDNN: the fused epilogue is LeakyReLU(0.01), got {act!r}")
        if int(rnn_layers) < 1 or int(dnn_blocks) < 0:
            raise ValueError(f"CRDNN: rnn_layers = {rnn_layers} must be >= 1 and dnn_blocks = {dnn_blocks} >= 0")
        self.rnn = LSTM(input_size=int(input_size), hidden_size=int(rnn_neurons), num_layers=int(rnn_layers),
                        batch_first=True, dropout=float(dropout) if int(rnn_layers) > 1 else 0.0,
                        bidirectional=bool(rnn_bidirectional))
        size = int(rnn_neurons) * (2 if rnn_bidirectional else 1)
        self.dnn = nn.ModuleList()
        for _ in range(int(dnn_blocks)):
            self.dnn.append(Linear(size, dnn_neurons, bias=True))
            size = int(dnn_neurons)
        self.output_size = size

    def forward(self, x):
        x = self.rnn(x.contiguous())[0]
        for lin in self.dnn:
            x = ops.linear(x, lin.w.weight, lin.w.bias, True)
        return x


class CNNFront(nn.Module):
    """The CRDNN lobe's CNN blocks and time pooling over the features [B, T, input_size] ->
    [B, T' , output_size], output_size = F_out * C_last (F halves, floor, in every block; T' = T // 2
    with time_pooling).  Parameters: block_{i}.conv_{j}.weight [C, Cin, 3, 3] / .bias [C],
    block_{i}.norm_{j}.weight / .bias [F_i, C] (torch's Conv2d / LayerNorm default init; the nn
    modules only hold them: the products run on the HIP kernels).  forward(x, keep=None): keep is
    one Dropout2d factor tensor [B, F_i // 2] (0 or 1 / (1 - p)) per block; by default it is drawn on
    the device from torch's generator when training and absent in eval mode."""

    def __init__(self, input_size, cnn_blocks=2, cnn_channels=(128, 256), cnn_kernelsize=(3, 3), dropout=0.15,
                 time_pooling=False):
        super().__init__()
        if tuple(int(k) for k in cnn_kernelsize) != (3, 3):
            raise ValueError(f"CNNFront: cnn_kernelsize = {tuple(cnn_kernelsize)}: only (3, 3) has a kernel")
        self.n_blocks, self.time_pooling, self.p = int(cnn_blocks), bool(time_pooling), float(dropout)
        if self.n_blocks < 0 or len(cnn_channels) < self.n_blocks or not 0.0 <= self.p < 1.0:
            raise ValueError(f"CNNFront: cnn_blocks = {cnn_blocks}, cnn_channels = {cnn_channels}, dropout = {dropout}")
        F, cin = int(input_size), 1
        for i in range(self.n_blocks):
            c = int(cnn_channels[i])
            if c % 16 or not 16 <= c <= 256:
                raise ValueError(f"CNNFront: cnn_channels[{i}] = {c} must be a multiple of 16 up to 256")
            if F < 2:
                raise ValueError(f"CNNFront: block {i} has {F} frequency bins left: nothing to pool")
            blk = nn.Module()
            blk.conv_1 = nn.Conv2d(cin, c, 3)
            blk.norm_1 = nn.LayerNorm([F, c])
            blk.conv_2 = nn.Conv2d(c, c, 3)
            blk.norm_2 = nn.LayerNorm([F, c])
            setattr(self, f"block_{i}", blk)
            F, cin = F // 2, c
        self.output_size = F * (cin if self.n_blocks else 1)

    def draw_keep(self, B, device):
        """One Dropout2d factor tensor per block, from torch's generator on `device`."""
        keep, F = [], None
        for i in range(self.n_blocks):
            F = getattr(self, f"block_{i}").norm_2.normalized_shape[0] // 2
            keep.append((torch.rand(B, F, device=device) >= self.p).to(torch.float32) / (1.0 - self.p))
        return keep

    def forward(self, x, keep=None):
        x = x.contiguous()
        if keep is None and self.training and self.p > 0.0:
            keep = self.draw_keep(x.shape[0], x.device)
        for i in range(self.n_blocks):
            blk = getattr(self, f"block_{i}")
            x = ops.conv2d_3x3(x, blk.conv_1.weight, blk.conv_1.bias)
            x = ops.layer_norm_fc_act(x, blk.norm_1.weight, blk.norm_1.bias)
            x = ops.conv2d_3x3(x, blk.conv_2.weight, blk.conv_2.bias)
            x = ops.layer_norm_fc_act(x, blk.norm_2.weight, blk.norm_2.bias, pool=True,
                                      keep=keep[i] if keep is not None else None)
        if self.time_pooling:
            x = ops.time_pool(x)
        return x.reshape(x.shape[0], x.shape[1], -1)


class ConvCRDNN(CRDNN):
    """CNNFront followed by CRDNN(input_size=front.output_size, cnn_blocks=0, time_pooling=False):
    the CRDNN keyword surface with the front end built.  With cnn_blocks = 0 and no time pooling it
    is CRDNN (the same parameters, the same forward)."""

    def __init__(self, input_size, activation=nn.LeakyReLU, dropout=0.15, cnn_blocks=2, cnn_channels=(128, 256),
                 cnn_kernelsize=(3, 3), time_pooling=False, rnn_layers=4, rnn_neurons=512, rnn_bidirectional=True,
                 dnn_blocks=2, dnn_neurons=512):
        front = None
        if int(cnn_blocks) > 0 or time_pooling:
            front = CNNFront(input_size, cnn_blocks, cnn_channels, cnn_kernelsize, dropout, time_pooling)
        super().__init__(front.output_size if front is not None else input_size, activation, dropout, 0,
                         cnn_channels, cnn_kernelsize, False, rnn_layers, rnn_neurons, rnn_bidirectional, dnn_blocks,
                         dnn_neurons)
        self.front = front

    def forward(self, x, keep=None):
        if self.front is not None:
            x = self.front(x, keep)
        return super().forward(x)
