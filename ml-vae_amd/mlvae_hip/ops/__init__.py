"""torch.autograd.Functions over libmlvae.so: the operator layer under the drop-in
nn.Modules (modules/fc_block.py, modules/vanilla_vae.py, modules/decoder.py), one module per
kernel family.  The package re-exports every name: callers write ops.<name>.

Every forward and backward below is a libmlvae.so launch on the current HIP stream; torch
only allocates the output tensors.  Inputs must be fp32 CUDA tensors (row-major [B, T, C]).
The fused training step (mlvae_hip/engine.py) uses the same kernels without autograd.
"""
from . import errors  # noqa: F401
from ._core import (  # noqa: F401
    colsum, current_shard, gemm, get_precision, _md_err, _need, _p, PREC, precision, raise_err, _rows,
    set_precision, shard, valid_frames, _ws
)
from .errors import (  # noqa: F401
    ALIGN_ERR_BLANK, ALIGN_ERR_CLASS, ALIGN_ERR_SHORT, CTC_ERR_PAIR, FLVL_ERR_LABEL, PI_ERR_LABEL,
    SCORE_ERR_K, SCORE_ERR_SEGMENTS
)
from .dense import (  # noqa: F401
    conv1d, Conv1dFn, linear, LinearFn
)
from .crdnn import (  # noqa: F401
    Conv2d3x3Fn, conv2d_3x3, Conv2dFirstFn, layer_norm_fc_act, LayerNormFCActFn, time_pool, TimePoolFn
)
from .vae import (  # noqa: F401
    apply_weight, ApplyWeightFn, gmm_collapsed, GmmLatentFn, hvae_latent, HvaeLatentFn, LOSS, masked_mean,
    MaskedMeanFn, randn, recon_loss, ReconFn, RED, ReparamKLFn
)
from .rnn import (  # noqa: F401
    bilstm, lstm, lstm_full, lstm_pair, lstm_pair_ok, LSTMFn, LSTMPairFn
)
from .md import (  # noqa: F401
    boundary_heads, BoundaryHeadsFn, flvl_md_head, FlvlMdHeadFn, phn_bce, PhnBceFn, pi_nll, pi_sample,
    pi_sample_k, PiNllFn, PiSampleFn, PiSampleKFn, raise_flvl_err, _raise_md, raise_pi_err, sfl_losses,
    SflLossesFn
)
from .scoring import (  # noqa: F401
    boundary_counts, boundary_topk, phn_acc_counts, raise_score_err
)
from .lattice import (  # noqa: F401
    align_counts, center_log_softmax, CenterLogSoftmaxFn, ctc_greedy_decode, ctc_md_counts, ctc_nll,
    ctc_viterbi, edit_align, hmm_forward, hmm_viterbi, LatticeFn, log_softmax, LogSoftmaxFn,
    raise_align_err, raise_ctc_eval_err, TOPO_CTC, TOPO_HMM
)
from .features import (  # noqa: F401
    cmvn_accumulate, cmvn_apply, fbank, kaldi_fbank, _raise_cmvn
)
from .w2v import (  # noqa: F401
    w2v_attention, w2v_attention_bwd, w2v_attention_supported, w2v_attention_train, w2v_cast, w2v_colsum,
    w2v_conv0, w2v_conv0_bwd, w2v_conv_dw, w2v_conv_dx, w2v_conv_dx_weights, w2v_conv_gemm, w2v_conv_pad, w2v_gemm,
    w2v_linear, w2v_linear_dw, w2v_linear_dx, w2v_norm_bwd,
    w2v_pos_conv, w2v_pos_conv_dw, w2v_pos_conv_dx, w2v_regroup, w2v_rows, w2v_rows_bwd, w2v_scale_shift,
    w2v_tensor_stats, W2VConvFn, W2VHeadFn, W2VLayerFn, W2VTailFn
)
