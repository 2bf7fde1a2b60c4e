"""CRDNN on the HIP stack: the keyword surface of speechbrain.lobes.models.CRDNN.CRDNN that the
CRDNN_CTC recipes' yaml passes (ref:src/models/CRDNN_CTC/model.yaml:23-35), built from what this
project has -- ``rnn``: modules.lstm.LSTM (``rnn_layers`` layers of ``rnn_neurons`` units,
bidirectional or not, inter-layer dropout, the persistent HIP recurrence), then ``dnn``:
``dnn_blocks`` times a Linear(bias=True) to ``dnn_neurons`` with LeakyReLU(0.01) fused into the
GEMM epilogue.

Limits, stated rather than approximated: ``cnn_blocks > 0`` and ``time_pooling=True`` raise
NotImplementedError -- the SpeechBrain lobe's Conv2d / LayerNorm / pooling front is not
reproduced; nor are its LiGRU (the recurrent layer here is an LSTM), the BatchNorm and the dropout
inside its DNN blocks.  ``cnn_channels`` and ``cnn_kernelsize`` are accepted and unused.  As with
every other SpeechBrain lobe in this project, parity with the lobe is unpinned."""
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
