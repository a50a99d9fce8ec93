"""Thin Python functions over the C ABI (include/dic.h).  torch is used only for device memory and
streams; every number is produced by libdic_hip.so.  Nothing here falls back to torch ops.

One module per family; every public name is re-exported here, and callers import from here."""
import ctypes as C          # (native.C: tests set restypes through it)

from .. import _lib
from .._lib import check, ptr, stream_ptr
from ._core import D_ATT, D_EMB, D_ENC, D_HID, DEFAULT_CONV_MODE, L_CELLS, L_COMPACT, batch_sizes_of
from .decode import (COMBINE_MODES, decoder_beam, decoder_beam_constrained, decoder_beam_diverse, decoder_beam_ensemble, decoder_beam_hard, decoder_greedy,
                     decoder_sample,
                     decoder_sample_constrained, decoder_sample_hard, decoder_score, decoder_score_hard, nic_beam, nic_greedy,
                     nic_sample, nic_score, token_ban_mask)
from .decoder import (DECODER_FIELDS, SCHEDULED_PICKS, STATES_GRAD_KEYS, DecoderPtrs, DecoderTape, HardStatesTape, StatesTape, attention_backward,
                      attention_forward, decoder_attention_relu_mask, decoder_backward, decoder_forward, decoder_forward_scheduled,
                      decoder_ptrs, decoder_states_backward,
                      decoder_states_backward_into, decoder_states_forward, decoder_states_hard_backward,
                      decoder_states_hard_backward_into, decoder_states_hard_forward)
from .encoders import (CONV_MODES, DEPTH_FIELDS, ConvBnLayer, DepthBnState, DepthPtrs, DepthTape, ResNetRunner, depth_encoder_backward,
                       depth_encoder_decisions, depth_encoder_forward, depth_ptrs, depth_status_word, f16x2_weight_scale)
from .nic import (NIC_EMB, NIC_FIELDS, NIC_STATES_GRAD_KEYS, NicPtrs, NicStatesTape, NicTape, nic_backward, nic_forward,
                  nic_head_backward, nic_head_forward, nic_pack_targets, nic_ptrs, nic_shapes, nic_states_backward,
                  nic_states_forward)
from .train_ops import (GRAD_NORM_MAX_SPANS, GRAD_NORM_PASS, GRAD_NORM_SCRATCH_BYTES, adamw_step, adamw_step_clipped, bleu,
                        bn_ema_update, caption_lengths, caption_loss, caption_loss_smoothed, check_label_smoothing, cider_d,
                        dropout_advance, dropout_draw, dropout_mask, gather_rows, grad_norm, pack_targets, rouge_l, scst_loss,
                        token_logprobs, token_logprobs_bwd, token_logprobs_bwd_into, token_mean_logit, token_mean_logit_bwd)

# which of dic_struct_bytes -> the ctypes mirror of that struct of include/dic.h (_core._load checks them all, once, and reads both names from here)
STRUCT_MIRRORS = ((0, ConvBnLayer), (1, DecoderPtrs), (2, DecoderPtrs), (3, DepthPtrs), (4, DepthPtrs), (5, DepthBnState),
                  (6, NicPtrs), (7, NicPtrs))
_mirrors_checked = False
