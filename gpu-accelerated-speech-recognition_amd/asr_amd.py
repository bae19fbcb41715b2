"""Python host mirror of the reference's C++ API over libasr_amd.so (ctypes).

The reference (jrxk/GPU-Accelerated-Speech-Recognition) exposes C++ classes
only; its callers are main.cpp / nn_test.cpp.  This module mirrors those
classes for Python callers, tests and bench.py, calling the C ABI of
include/asr_amd.h — it contains no arithmetic of its own:

    CTCBeamSearch(vocab, vocabSize, beamWidth, blankID)   CTCBeamSearch.h:107
        .decode(seqProb, timestep, batchSize)             CTCBeamSearch.cu:262
    Linear(batch_size, input_size, output_size).forward   Linear.cu:42
    RNN_Cell(batch, in, hidden).forward                   RNN_Cell.cu:65
    RNN(batch, in, hidden, time_step, num_layers).forward RNN.cu:9
    DeviceMatrix ~ cuMatrix<float> (toGpu / toCpu)        cuMatrix.h:72-105
    ctc_score(emis, targets) / ctc_align(emis, targets)
                                          exact CTC log-likelihood and forced
                                          alignment of given transcripts
                                          (asr_ctc_align); no reference member
    LSTM(input_size, hidden_size, num_layers, bidirectional).forward
                                          torch.nn.LSTM; no reference member
    GRU(input_size, hidden_size, num_layers, bidirectional).forward
                                          torch.nn.GRU; no reference member
    Conv1d(c_in, c_out, kernel, stride, dilation, padding, groups, act).forward
                                          torch.nn.Conv1d over time, time-major,
                                          bias and activation fused
                                          (asr_conv1d_fwd); no reference member
    Conv2d.from_torch(conv, bn, act, feat_in=F).forward
    Conv2dSubsampling.from_torch(conv, out, feat_in, scale).forward
                                          torch.nn.Conv2d over (time, frequency),
                                          time-major with the frequency axis inside
                                          the row (asr_conv2d_fwd), and the
                                          Conv2dSubsampling front end of Conformer
                                          encoders; no reference member
    MultiheadAttention.from_torch(mha, chunk, left, right).forward
    LayerNorm.from_torch(ln).forward / TransformerEncoderLayer.from_torch(layer).forward
                                          torch.nn.MultiheadAttention (self-attention
                                          with lengths and a chunked window),
                                          LayerNorm and TransformerEncoderLayer,
                                          time-major (asr_attention_fwd,
                                          asr_layernorm_fwd); no reference member
    ConformerLayer.from_torch(ffn1=..., attn=..., conv=..., ffn2=..., final_norm=...).forward
    ConformerConv.from_torch(norm, pw1, dw, bn, pw2).forward / Conformer(layers).forward
                                          a Conformer encoder block, time-major:
                                          SiLU feed-forwards (EPI_BIAS_SILU),
                                          attention, and the convolution module
                                          with GLU -> depthwise -> BatchNorm ->
                                          SiLU in one launch (asr_glu_dwconv_fwd);
                                          no reference member
    TransformerDecoder.from_torch(embedding, decoder, output).score(hyps, utt, memory, T, B)
    attention_rescore(nbest, decoder, memory, T, B) / CTCDecoder.attention_rescore(...)
                                          attention-decoder rescoring of an n-best:
                                          causal self-attention, grouped
                                          cross-attention over each hypothesis's own
                                          utterance (asr_cross_attention_fwd) and
                                          the token scores (asr_token_score); the
                                          embedding is gathered on the device
                                          (asr_embed_fwd); no reference member
    TransformerDecoder.beam_search(memory, T, B, enc_lengths, beam=10) / .greedy(...)
    TransformerDecoder.begin(...) / .step(state) / .prune(state, logp)
                                          attention-decoder beam search on a K/V
                                          cache read through an ancestry table
                                          (asr_decode_attention_fwd), the exact
                                          top-K prune and reorder in one launch
                                          (asr_attn_beam_step, host twin
                                          asr_attn_beam_step_host); no reference
                                          member
    FeatureFrontend(sample_rate=..., n_mfcc=..., n_context=...).forward
                                          waveform -> log-mel / MFCC features
                                          (asr_fbank_*); no reference member
    NGramLM.from_arpa(path).score(token_lists) / CTCDecoder.lm_rescore(...)
                                          back-off n-gram LM scoring and n-best
                                          rescoring (asr_lm_*); no reference member
    CTCLMDecoder(V, beam_width, lm, tok_of_label, alpha, beta).decode(emis)
                                          beam search with the n-gram LM fused into
                                          every prune (asr_ctc_lm_*); no reference
                                          member
    CTCLMDecoder.word(V, beam_width, lm, Lexicon.from_lm(lm, labels), alpha, beta)
                                          the same search with a word-level LM fused
                                          through a lexicon trie (asr_lexicon_*,
                                          asr_ctc_lm_create_word); no reference member
    TransducerDecoder.from_torch(embedding, lstm, enc_proj, pred_proj, out_proj, blank).decode(enc)
                                          RNN-T greedy decoding, the whole (t, u)
                                          walk in one launch (asr_rnnt_*); no
                                          reference member
    TransducerDecoder.beam_search(enc, beam=4)
                                          RNN-T beam search, one symbol per frame,
                                          the n-best in one launch (asr_rnnt_beam*);
                                          no reference member
    TransducerDecoder.beam_search(enc, beam=4, lm=NGramLM, alpha=.., beta=.., tok_of_label=..)
                                          the same search with the n-gram LM fused
                                          into every prune (asr_rnnt_lm_*,
                                          asr_rnnt_beam_lm*); no reference member
    TransducerDecoder.score(enc, targets) / .align(enc, targets) / .rescore(nbest, enc)
                                          exact transducer log-likelihood, best
                                          alignment and emission frames of given
                                          transcripts, the joint fused over the
                                          (t, u) grid (asr_rnnt_align*); no
                                          reference member

The native library is required: importing this module on a machine where
libasr_amd.so is missing raises, there is no fallback path.
"""
from __future__ import annotations

import collections
import ctypes
import math
import os
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
# ASR_LIB selects a diagnostic variant (e.g. libasr_amd_stamps.so) for tools/.
LIB_PATH = PKG_DIR / os.environ.get("ASR_LIB", "libasr_amd.so")

ASR_OK = 0
ASR_ERR_ARG = 1
ASR_ERR_HIP = 2
ASR_ERR_OOM = 3
ASR_ERR_BEAM_OVERFLOW = 4
ASR_ERR_UNSUPPORTED = 5
ASR_ERR_STATE = 6
ASR_ERR_INTERNAL = 7

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_LOGSOFTMAX, EPI_BIAS_SILU = 0, 1, 2, 3, 4
SEMANTICS_CPU, SEMANTICS_CUDA = 0, 1   # asr_ctc_set_semantics
ASR_CTC_WAVES_LIST = -1                # asr_ctc_set_waves: the one-wave list kernel
ASR_CTC_TS_MAX_T = 65536               # longest decode with timesteps on (16-bit frames)

# Every symbol include/asr_amd.h declares (checked by tests/test_boundary.py).
EXPORTS = [
    "asr_status_string", "asr_version", "asr_get_device_count", "asr_set_device",
    "asr_get_device", "asr_device_malloc", "asr_device_free", "asr_host_malloc",
    "asr_host_free", "asr_memcpy_h2d", "asr_memcpy_d2h", "asr_memcpy_d2d", "asr_memset",
    "asr_stream_create", "asr_stream_destroy", "asr_stream_sync", "asr_device_sync",
    "asr_matmul", "asr_matmul_ta", "asr_matmul_tb", "asr_matadd", "asr_linear_fwd",
    "asr_rnn_cell_fwd", "asr_rnn_fwd", "asr_rnn_recur_fwd", "asr_rnn_persist_stats", "asr_rnn_emit_fwd", "asr_rnn_bidir_workspace_bytes", "asr_rnn_bidir_fwd",
    "asr_lstm_workspace_bytes", "asr_lstm_fwd", "asr_lstm_recur_fwd",
    "asr_gru_workspace_bytes", "asr_gru_fwd", "asr_gru_recur_fwd",
    "asr_conv1d_out_frames", "asr_conv1d_fwd", "asr_glu_dwconv_fwd",
    "asr_conv2d_out_frames", "asr_conv2d_out_feats", "asr_conv2d_fwd",
    "asr_attention_fwd", "asr_layernorm_fwd", "asr_mask_rows",
    "asr_cross_attention_fwd", "asr_token_score",
    "asr_decode_attention_fwd", "asr_embed_fwd", "asr_attn_beam_step", "asr_attn_beam_step_host",
    "asr_fbank_num_frames", "asr_fbank_feature_dim", "asr_fbank_host_tables", "asr_fbank_create",
    "asr_fbank_destroy", "asr_fbank_workspace_bytes", "asr_fbank_fwd",
    "asr_lm_create_arpa", "asr_lm_create_arpa_mem", "asr_lm_destroy", "asr_lm_get_info", "asr_lm_token_id",
    "asr_lm_token_string", "asr_lm_score_host", "asr_lm_upload", "asr_lm_score",
    "asr_edit_distance", "asr_edit_distance_host", "asr_nbest_mbr", "asr_nbest_mbr_host",
    "asr_ctc_lm_create", "asr_ctc_lm_destroy", "asr_ctc_lm_decode", "asr_ctc_lm_decode_host",
    "asr_ctc_lm_get_beams", "asr_ctc_lm_get_best", "asr_ctc_lm_host_gaps",
    "asr_lexicon_create", "asr_lexicon_upload", "asr_lexicon_get_info", "asr_lexicon_destroy",
    "asr_ctc_lm_create_word",
    "asr_rnnt_create", "asr_rnnt_upload", "asr_rnnt_get_info", "asr_rnnt_destroy", "asr_rnnt_workspace_bytes",
    "asr_rnnt_greedy", "asr_rnnt_greedy_host",
    "asr_rnnt_beam_workspace_bytes", "asr_rnnt_beam", "asr_rnnt_beam_host",
    "asr_rnnt_lm_create", "asr_rnnt_lm_destroy", "asr_rnnt_beam_lm_workspace_bytes", "asr_rnnt_beam_lm",
    "asr_rnnt_beam_lm_host",
    "asr_rnnt_align_workspace_bytes", "asr_rnnt_align", "asr_rnnt_align_host",
    "asr_ctc_create", "asr_ctc_destroy", "asr_ctc_decode",
    "asr_ctc_get_best", "asr_ctc_get_beams", "asr_ctc_last_kernel_ms", "asr_ctc_set_waves",
    "asr_ctc_get_config", "asr_ctc_decode_ex", "asr_ctc_decode_segment", "asr_ctc_set_semantics",
    "asr_ctc_set_timesteps", "asr_ctc_get_beams_ts", "asr_ctc_set_result_stream",
    "asr_ctc_set_concurrency", "asr_ctc_align_workspace_bytes", "asr_ctc_align",
    "asr_rnn_set_recurrence", "asr_rnn_get_recurrence",
    "asr_set_dense_arith", "asr_get_dense_arith",
    "asr_pipeline_create", "asr_pipeline_submit", "asr_pipeline_collect", "asr_pipeline_pending",
    "asr_pipeline_describe", "asr_pipeline_get_production", "asr_pipeline_get_streams", "asr_pipeline_get_queue_use",
    "asr_pipeline_peek_emissions", "asr_pipeline_get_segments", "asr_pipeline_get_drain", "asr_pipeline_get_groups",
    "asr_pipeline_get_placement", "asr_pipeline_probe_placement", "asr_pipeline_set_timing",
    "asr_pipeline_get_timeline", "asr_pipeline_destroy", "asr_pipeline_create_coalesced", "asr_pipeline_get_coalesce",
]
# asr_pipeline_get_placement roles (ASR_PIPE_ROLE_*)
PIPE_ROLES = {0: "decode", 1: "production", 2: "decode_cu_gemm", 3: "gemm"}
ASR_MAX_XCC = 16


class AsrError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: {status_string(status)} (status {status})")


_lib: Optional[ctypes.CDLL] = None
_vp = ctypes.c_void_p
_i = ctypes.c_int
_sz = ctypes.c_size_t
_f = ctypes.c_float


def lib() -> ctypes.CDLL:
    """Load libasr_amd.so (built by `make` in this directory)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} not found: build it with __graft_entry__.build() "
                           "or `make -C gpu-accelerated-speech-recognition_amd`")
    L = ctypes.CDLL(str(LIB_PATH))
    L.asr_status_string.restype = ctypes.c_char_p
    L.asr_status_string.argtypes = [_i]
    L.asr_version.restype = ctypes.c_char_p
    sig = {
        "asr_get_device_count": [ctypes.POINTER(_i)],
        "asr_set_device": [_i],
        "asr_get_device": [ctypes.POINTER(_i)],
        "asr_device_malloc": [ctypes.POINTER(_vp), _sz],
        "asr_device_free": [_vp],
        "asr_host_malloc": [ctypes.POINTER(_vp), _sz],
        "asr_host_free": [_vp],
        "asr_memcpy_h2d": [_vp, _vp, _sz, _vp],
        "asr_memcpy_d2h": [_vp, _vp, _sz, _vp],
        "asr_memcpy_d2d": [_vp, _vp, _sz, _vp],
        "asr_memset": [_vp, _i, _sz, _vp],
        "asr_stream_create": [ctypes.POINTER(_vp)],
        "asr_stream_destroy": [_vp],
        "asr_stream_sync": [_vp],
        "asr_device_sync": [],
        "asr_matmul": [_vp, _vp, _vp, _i, _i, _i, _vp],
        "asr_matmul_ta": [_vp, _vp, _vp, _i, _i, _i, _vp],
        "asr_matmul_tb": [_vp, _vp, _vp, _i, _i, _i, _vp],
        "asr_matadd": [_vp, _vp, _vp, _i, _i, _f, _vp],
        "asr_linear_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "asr_rnn_cell_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
        "asr_rnn_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "asr_rnn_recur_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
        "asr_rnn_persist_stats": [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)],
        "asr_rnn_set_recurrence": [_i],
        "asr_rnn_get_recurrence": [ctypes.POINTER(_i)],
        "asr_set_dense_arith": [_i],
        "asr_get_dense_arith": [ctypes.POINTER(_i)],
        "asr_rnn_emit_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "asr_pipeline_create": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp)],
        "asr_pipeline_create_coalesced": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp)],
        "asr_pipeline_get_coalesce": [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)],
        "asr_pipeline_submit": [_vp, _vp],
        "asr_pipeline_collect": [_vp, _vp, _i, _vp, _vp, _vp],
        "asr_pipeline_pending": [_vp, ctypes.POINTER(_i)],
        "asr_pipeline_describe": [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i),
                                  ctypes.POINTER(_i)],
        "asr_pipeline_destroy": [_vp],
        "asr_pipeline_get_production": [_vp, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong),
                                        ctypes.POINTER(_i)],
        "asr_pipeline_get_streams": [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i)],
        "asr_pipeline_get_queue_use": [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i)],
        "asr_pipeline_get_placement": [_vp, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i),
                                       ctypes.POINTER(_i)],
        "asr_pipeline_probe_placement": [_vp, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)],
        "asr_pipeline_set_timing": [_vp, _i],
        "asr_pipeline_get_timeline": [_vp, _i, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_longlong),
                                      ctypes.POINTER(_f)],
        "asr_pipeline_peek_emissions": [_vp, ctypes.POINTER(_vp)],
        "asr_pipeline_get_segments": [_vp, ctypes.POINTER(_i)],
        "asr_pipeline_get_drain": [_vp, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_double)],
        "asr_pipeline_get_groups": [_vp, ctypes.POINTER(_i)],
        "asr_rnn_bidir_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
        "asr_lstm_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp,
                         _i, _i, _i, _i, _i, _vp],
        "asr_lstm_recur_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp,
                               _i, _i, _i, _i, _vp],
        "asr_gru_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, _vp, _vp,
                        _i, _i, _i, _i, _i, _vp],
        "asr_gru_recur_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, _vp, _i, _i, _i, _i, _vp],
        "asr_conv1d_out_frames": [_vp, _i],
        "asr_conv1d_fwd": [_vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, _i, _i, _vp],
        "asr_conv2d_out_frames": [_vp, _i],
        "asr_conv2d_out_feats": [_vp],
        "asr_conv2d_fwd": [_vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, _i, _i, _vp],
        "asr_glu_dwconv_fwd": [_vp, _vp, ctypes.c_long, _vp, _vp, _vp, _vp, ctypes.c_long, _i, _i, _vp],
        "asr_attention_fwd": [_vp, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp,
                              ctypes.c_long, _i, _i, _i, _i, _i, _vp],
        "asr_layernorm_fwd": [_vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, _f, _vp, _vp, ctypes.c_long,
                              _i, _i, _i, _vp],
        "asr_mask_rows": [_vp, ctypes.c_long, _vp, _i, _i, _i, _vp],
        "asr_cross_attention_fwd": [_vp, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, _vp,
                                    _i, _vp, ctypes.c_long, _i, _i, _i, _i, _vp],
        "asr_token_score": [_vp, ctypes.c_long, _vp, _vp, _vp, _i, _i, _i, _vp],
        "asr_decode_attention_fwd": [_vp, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp,
                                     ctypes.c_long, _vp, _vp, ctypes.c_long, _i, _i, _i, _vp],
        "asr_embed_fwd": [_vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, ctypes.c_double, _vp, ctypes.c_long,
                          _i, _i, _i, _i, _vp],
        "asr_attn_beam_step": [_vp, _vp, ctypes.c_long] + [_vp] * 12,
        "asr_attn_beam_step_host": [_vp, _vp, ctypes.c_long] + [_vp] * 11,
        "asr_fbank_num_frames": [_vp, _i],
        "asr_fbank_feature_dim": [_vp],
        "asr_fbank_host_tables": [_vp, _vp, _vp, _vp],
        "asr_fbank_create": [_vp, ctypes.POINTER(_vp)],
        "asr_fbank_destroy": [_vp],
        "asr_fbank_fwd": [_vp, _vp, ctypes.c_long, _vp, _i, _i, _vp, ctypes.c_long, _vp, _vp, _i, _vp],
        "asr_lm_create_arpa": [ctypes.c_char_p, _f, ctypes.POINTER(_vp)],
        "asr_lm_create_arpa_mem": [ctypes.c_char_p, _sz, _f, ctypes.POINTER(_vp)],
        "asr_lm_destroy": [_vp],
        "asr_lm_get_info": [_vp, _vp],
        "asr_lm_token_id": [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)],
        "asr_lm_token_string": [_vp, ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p)],
        "asr_lm_score_host": [_vp, _vp, ctypes.c_long, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_long],
        "asr_lm_upload": [_vp],
        "asr_lm_score": [_vp, _vp, ctypes.c_long, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_long, _vp],
        "asr_edit_distance": [_vp, ctypes.c_long, _vp, _i, _i, _vp, ctypes.c_long, _vp, _i, _i, _vp, _vp, _i, _vp, _vp,
                              _vp],
        "asr_edit_distance_host": [_vp, ctypes.c_long, _vp, _i, _i, _vp, ctypes.c_long, _vp, _i, _i, _vp, _vp, _i, _vp,
                                   _vp],
        "asr_nbest_mbr": [_vp, ctypes.c_long, _vp, _i, _i, _vp, _i, _i, _vp, _vp, ctypes.c_long, _vp, _vp, _vp],
        "asr_nbest_mbr_host": [_vp, ctypes.c_long, _vp, _i, _i, _vp, _i, _i, _vp, _vp, ctypes.c_long, _vp, _vp],
        "asr_ctc_lm_create": [_vp, _i, _i, _i, _i, _vp, _vp, _f, _f, _i, _i, ctypes.POINTER(_vp)],
        "asr_ctc_lm_destroy": [_vp],
        "asr_ctc_lm_decode": [_vp, _vp, _i, _i, ctypes.c_long, ctypes.c_long, _vp, _i, _vp],
        "asr_ctc_lm_decode_host": [_vp, _vp, _i, _i, ctypes.c_long, ctypes.c_long, _vp, _i],
        "asr_ctc_lm_get_beams": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "asr_ctc_lm_get_best": [_vp, _vp, _i, _vp, _vp],
        "asr_ctc_lm_host_gaps": [_vp, _vp],
        "asr_lexicon_create": [_vp, _vp, _vp, _i, _i, _i, ctypes.POINTER(_vp)],
        "asr_lexicon_upload": [_vp],
        "asr_lexicon_get_info": [_vp, _vp],
        "asr_lexicon_destroy": [_vp],
        "asr_ctc_lm_create_word": [_vp, _i, _i, _i, _i, _vp, _vp, _f, _f, _i, _i, _i, ctypes.POINTER(_vp)],
        "asr_rnnt_create": [_vp, _vp, ctypes.POINTER(_vp)],
        "asr_rnnt_upload": [_vp],
        "asr_rnnt_get_info": [_vp, _vp],
        "asr_rnnt_destroy": [_vp],
        "asr_rnnt_greedy": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "asr_rnnt_greedy_host": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "asr_rnnt_beam": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "asr_rnnt_beam_host": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
        "asr_rnnt_lm_create": [_vp, _vp, _vp, _f, _f, _i, ctypes.POINTER(_vp)],
        "asr_rnnt_lm_destroy": [_vp],
        "asr_rnnt_beam_lm": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "asr_rnnt_beam_lm_host": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "asr_rnnt_align": [_vp, _vp, _vp, _i, _i, _vp, ctypes.c_long, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
        "asr_rnnt_align_host": [_vp, _vp, _vp, _i, _i, _vp, ctypes.c_long, _vp, _vp, _i, _i, _i, _vp, _vp, _vp],
        "asr_ctc_create": [_vp, _i, _i, _i, _i, ctypes.POINTER(_vp)],
        "asr_ctc_destroy": [_vp],
        "asr_ctc_decode": [_vp, _vp, _i, _i, _i, _vp],
        "asr_ctc_get_best": [_vp, _vp, _i, _vp, _vp],
        "asr_ctc_get_beams": [_vp, _i, _i, _vp, _vp, _vp, _vp],
        "asr_ctc_last_kernel_ms": [_vp, ctypes.POINTER(_f)],
        "asr_ctc_set_waves": [_vp, _i],
        "asr_ctc_set_concurrency": [_vp, _i],
        "asr_ctc_get_config": [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)],
        "asr_ctc_decode_ex": [_vp, _vp, _i, _i, ctypes.c_long, ctypes.c_long, _vp, _i, _vp],
        "asr_ctc_decode_segment": [_vp, _vp, _i, _i, _i, _i, ctypes.c_long, ctypes.c_long, _vp, _i, _vp],
        "asr_ctc_set_semantics": [_vp, _i],
        "asr_ctc_set_timesteps": [_vp, _i],
        "asr_ctc_set_result_stream": [_vp, _vp],
        "asr_ctc_get_beams_ts": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp],
        "asr_ctc_align": [_vp, _i, _i, _i, ctypes.c_long, ctypes.c_long, _vp, _i, _i, _vp, ctypes.c_long, _vp, _vp,
                          _i, _i, _vp, _vp, _vp, ctypes.c_long, _vp, _vp, _vp],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = _i
    L.asr_rnn_bidir_workspace_bytes.argtypes = [_i, _i, _i]
    L.asr_rnn_bidir_workspace_bytes.restype = _sz
    L.asr_lstm_workspace_bytes.argtypes = [_i, _i, _i]
    L.asr_lstm_workspace_bytes.restype = _sz
    L.asr_gru_workspace_bytes.argtypes = [_i, _i, _i]
    L.asr_gru_workspace_bytes.restype = _sz
    L.asr_fbank_workspace_bytes.argtypes = [_vp, _i, _i]
    L.asr_fbank_workspace_bytes.restype = _sz
    L.asr_ctc_align_workspace_bytes.argtypes = [_i, _i, _i]
    L.asr_ctc_align_workspace_bytes.restype = _sz
    L.asr_rnnt_workspace_bytes.argtypes = [_vp, _i, _i]
    L.asr_rnnt_workspace_bytes.restype = _sz
    L.asr_rnnt_beam_workspace_bytes.argtypes = [_vp, _i, _i, _i]
    L.asr_rnnt_beam_workspace_bytes.restype = _sz
    L.asr_rnnt_beam_lm_workspace_bytes.argtypes = [_vp, _i, _i, _i]
    L.asr_rnnt_beam_lm_workspace_bytes.restype = _sz
    L.asr_rnnt_align_workspace_bytes.argtypes = [_vp, _i, _i, _i, _i]
    L.asr_rnnt_align_workspace_bytes.restype = _sz
    _lib = L
    return L


def status_string(status: int) -> str:
    return lib().asr_status_string(status).decode()


def check(rc: int, what: str) -> None:
    if rc != ASR_OK:
        raise AsrError(rc, what)


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def device_count() -> int:
    n = _i(0)
    check(lib().asr_get_device_count(ctypes.byref(n)), "asr_get_device_count")
    return n.value


def set_device(d: int) -> None:
    check(lib().asr_set_device(d), "asr_set_device")


def synchronize() -> None:
    check(lib().asr_device_sync(), "asr_device_sync")


class DeviceMatrix:
    """fp32 row-major device buffer (cuMatrix<float> device side)."""

    def __init__(self, rows: int, cols: int = 1, data: Optional[np.ndarray] = None):
        self.rows, self.cols = int(rows), int(cols)
        self.nbytes = 4 * self.rows * self.cols
        p = _vp()
        check(lib().asr_device_malloc(ctypes.byref(p), self.nbytes), "asr_device_malloc")
        self.ptr = p.value or 0
        if data is not None:
            self.toGpu(data)

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DeviceMatrix":
        a = np.ascontiguousarray(a, dtype=np.float32)
        r = a.shape[0] if a.ndim else 1
        return cls(r, a.size // max(r, 1), a)

    def toGpu(self, a: np.ndarray, stream: int = 0) -> None:
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.size * 4 == self.nbytes, (a.shape, self.rows, self.cols)
        check(lib().asr_memcpy_h2d(self.ptr, _ptr(a), self.nbytes, stream), "asr_memcpy_h2d")

    def toCpu(self, stream: int = 0) -> np.ndarray:
        out = np.empty((self.rows, self.cols), dtype=np.float32)
        check(lib().asr_memcpy_d2h(_ptr(out), self.ptr, self.nbytes, stream), "asr_memcpy_d2h")
        return out

    def free(self) -> None:
        if self.ptr:
            lib().asr_device_free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBytes:
    """Untyped device allocation (workspace / generic buffers)."""

    def __init__(self, nbytes: int):
        p = _vp()
        check(lib().asr_device_malloc(ctypes.byref(p), int(nbytes)), "asr_device_malloc")
        self.ptr, self.nbytes = p.value or 0, int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                lib().asr_device_free(self.ptr)
        except Exception:
            pass


# --------------------------------------------------------------------- dense
def linear_fwd(x: DeviceMatrix, W: DeviceMatrix, b: Optional[DeviceMatrix], y: DeviceMatrix,
               epilogue: int = EPI_BIAS_RELU, stream: int = 0) -> DeviceMatrix:
    M, K = x.rows, x.cols
    N = W.cols
    assert W.rows == K and y.rows == M and y.cols == N
    check(lib().asr_linear_fwd(x.ptr, W.ptr, b.ptr if b else None, y.ptr, M, K, N, epilogue,
                               stream), "asr_linear_fwd")
    return y


def rnn_fwd(x: DeviceMatrix, W_ih: DeviceMatrix, W_hh: DeviceMatrix, b_ih: DeviceMatrix,
            b_hh: DeviceMatrix, hid: DeviceMatrix, T: int, B: int,
            h0: Optional[DeviceMatrix] = None, stream: int = 0) -> DeviceMatrix:
    inp, H = W_ih.rows, W_ih.cols
    check(lib().asr_rnn_fwd(x.ptr, h0.ptr if h0 else None, W_ih.ptr, W_hh.ptr, b_ih.ptr,
                            b_hh.ptr, hid.ptr, T, B, inp, H, stream), "asr_rnn_fwd")
    return hid


def rnn_recur_fwd(W_hh: DeviceMatrix, b_ih: DeviceMatrix, b_hh: DeviceMatrix, hid: DeviceMatrix,
                  T: int, B: int, h0: Optional[DeviceMatrix] = None, stream: int = 0) -> DeviceMatrix:
    """The recurrence stage alone (asr_rnn_recur_fwd): hid holds x.W_ih on entry,
    the hidden states on return."""
    H = W_hh.cols
    check(lib().asr_rnn_recur_fwd(h0.ptr if h0 else None, W_hh.ptr, b_ih.ptr, b_hh.ptr, hid.ptr,
                                  T, B, H, stream), "asr_rnn_recur_fwd")
    return hid


def rnn_persist_stats() -> tuple:
    """(launches, recoveries) of the one-launch H > 256 recurrence in this
    process (asr_rnn_persist_stats): recoveries are launches that gave up
    waiting for their workgroups and were finished by the recovery kernel."""
    n, r = ctypes.c_longlong(0), ctypes.c_longlong(0)
    check(lib().asr_rnn_persist_stats(ctypes.byref(n), ctypes.byref(r)), "asr_rnn_persist_stats")
    return n.value, r.value


def rnn_emit_fwd(W_hh: DeviceMatrix, b_ih: DeviceMatrix, b_hh: DeviceMatrix, W_out: DeviceMatrix,
                 b_out: DeviceMatrix, P: DeviceMatrix, emis: DeviceMatrix, T: int, B: int,
                 h0: Optional[DeviceMatrix] = None, hid: Optional[DeviceMatrix] = None,
                 stream: int = 0) -> DeviceMatrix:
    """Recurrence + emission projection + log_softmax in one kernel
    (asr_rnn_emit_fwd): P holds x.W_ih (unchanged), emis [T*B, V] receives the
    log-probabilities, hid (optional) the hidden states."""
    H, V = W_hh.cols, W_out.cols
    assert P.rows == T * B and P.cols == H and emis.rows == T * B and emis.cols == V
    check(lib().asr_rnn_emit_fwd(h0.ptr if h0 else None, W_hh.ptr, b_ih.ptr, b_hh.ptr, W_out.ptr,
                                 b_out.ptr, P.ptr, hid.ptr if hid else None, emis.ptr, T, B, H, V,
                                 stream), "asr_rnn_emit_fwd")
    return emis


def rnn_bidir_fwd(x: DeviceMatrix, params: Sequence[Tuple[DeviceMatrix, ...]], out: DeviceMatrix,
                  T: int, B: int, h0: Optional[DeviceMatrix] = None,
                  work: Optional["DeviceBytes"] = None, stream: int = 0) -> DeviceMatrix:
    """nn.RNN(bidirectional=True) (baseline/model.py:30): params[d] = (W_ih, W_hh,
    b_ih, b_hh) for d = 0 (forward in t) and d = 1 (reverse); h0 [2*B, H];
    out [T*B, 2H] = (h_fwd, h_bwd) per row."""
    inp, H = params[0][0].rows, params[0][0].cols
    assert len(params) == 2 and x.rows == T * B and x.cols == inp
    assert out.rows == T * B and out.cols == 2 * H
    need = lib().asr_rnn_bidir_workspace_bytes(T, B, H)
    if work is None or work.nbytes < need:
        work = DeviceBytes(need)
    arr = [(_vp * 2)(*(params[d][k].ptr for d in range(2))) for k in range(4)]
    check(lib().asr_rnn_bidir_fwd(x.ptr, h0.ptr if h0 else None, arr[0], arr[1], arr[2], arr[3],
                                  out.ptr, work.ptr, T, B, inp, H, stream), "asr_rnn_bidir_fwd")
    if stream == 0:
        check(lib().asr_stream_sync(None), "asr_stream_sync")
    return out


RNN_RECUR_AUTO, RNN_RECUR_VALU, RNN_RECUR_MFMA = 0, 1, 2


def rnn_set_recurrence(kind: int) -> None:
    """Process-wide recurrence kernel choice (asr_rnn_set_recurrence)."""
    check(lib().asr_rnn_set_recurrence(int(kind)), "asr_rnn_set_recurrence")


def rnn_get_recurrence() -> int:
    """The process-wide recurrence kernel choice (asr_rnn_get_recurrence)."""
    k = _i()
    check(lib().asr_rnn_get_recurrence(ctypes.byref(k)), "asr_rnn_get_recurrence")
    return k.value


DENSE_F32, DENSE_SPLIT_BF16 = 0, 1


def set_dense_arith(arith: int) -> None:
    """Process-wide arithmetic of the dense contractions (asr_set_dense_arith):
    DENSE_SPLIT_BF16 (default, fp32-accurate three-piece bf16 MFMA) or DENSE_F32."""
    check(lib().asr_set_dense_arith(int(arith)), "asr_set_dense_arith")


def get_dense_arith() -> int:
    a = _i()
    check(lib().asr_get_dense_arith(ctypes.byref(a)), "asr_get_dense_arith")
    return a.value


def rnn_cell_fwd(x: DeviceMatrix, h_prev: DeviceMatrix, W_ih: DeviceMatrix,
                 W_hh: DeviceMatrix, b_ih: DeviceMatrix, b_hh: DeviceMatrix,
                 h_out: DeviceMatrix, stream: int = 0) -> DeviceMatrix:
    B, inp = x.rows, x.cols
    H = W_ih.cols
    check(lib().asr_rnn_cell_fwd(x.ptr, h_prev.ptr, W_ih.ptr, W_hh.ptr, b_ih.ptr, b_hh.ptr,
                                 h_out.ptr, B, inp, H, stream), "asr_rnn_cell_fwd")
    return h_out


class Linear:
    """Linear.h: y = relu(x.W + b), W [in, out] row-major (Linear.cu:42-49)."""

    def __init__(self, batch_size: int, input_size: int, output_size: int,
                 weight: Optional[np.ndarray] = None, bias: Optional[np.ndarray] = None,
                 epilogue: int = EPI_BIAS_RELU):
        self.batch_size, self.input_size, self.output_size = batch_size, input_size, output_size
        w = np.zeros((input_size, output_size), np.float32) if weight is None else weight
        b = np.zeros((output_size,), np.float32) if bias is None else bias
        self.w = DeviceMatrix.from_numpy(np.asarray(w, np.float32).reshape(input_size, output_size))
        self.b = DeviceMatrix.from_numpy(np.asarray(b, np.float32).reshape(output_size, 1))
        self.outputs = DeviceMatrix(batch_size, output_size)
        self.epilogue = epilogue

    def forward(self, inputs: DeviceMatrix, stream: int = 0) -> DeviceMatrix:
        return linear_fwd(inputs, self.w, self.b, self.outputs, self.epilogue, stream)


class RNN:
    """RNN.h: tanh RNN, num_layers stacked, time-major [T*B, H] hiddens."""

    def __init__(self, batch_size: int, input_size: int, hidden_size: int, time_step: int,
                 num_layers: int = 1, params: Optional[Sequence[Tuple[np.ndarray, ...]]] = None):
        self.B, self.inp, self.H, self.T, self.L = batch_size, input_size, hidden_size, time_step, num_layers
        self.layers = []
        for l in range(num_layers):
            i = input_size if l == 0 else hidden_size
            if params is None:
                p = (np.zeros((i, hidden_size), np.float32), np.zeros((hidden_size, hidden_size), np.float32),
                     np.zeros(hidden_size, np.float32), np.zeros(hidden_size, np.float32))
            else:
                p = params[l]
            w_ih, w_hh, b_ih, b_hh = (DeviceMatrix.from_numpy(np.asarray(a, np.float32).reshape(
                (i, hidden_size) if k == 0 else (hidden_size, hidden_size) if k == 1 else (hidden_size, 1)))
                for k, a in enumerate(p))
            self.layers.append((w_ih, w_hh, b_ih, b_hh))
        self.hiddens = [DeviceMatrix(time_step * batch_size, hidden_size) for _ in range(num_layers)]

    def forward(self, inputs: DeviceMatrix, stream: int = 0) -> DeviceMatrix:
        x = inputs
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self.layers):
            rnn_fwd(x, w_ih, w_hh, b_ih, b_hh, self.hiddens[l], self.T, self.B, None, stream)
            x = self.hiddens[l]
        return self.hiddens[-1]


# ---------------------------------------------------------------- LSTM / GRU
def lstm_workspace_bytes(T: int, B: int, H: int) -> int:
    """asr_lstm_workspace_bytes: 0 for a shape the LSTM kernels do not take."""
    return int(lib().asr_lstm_workspace_bytes(T, B, H))


def gru_workspace_bytes(T: int, B: int, H: int) -> int:
    """asr_gru_workspace_bytes: 0 for a shape the GRU kernels do not take."""
    return int(lib().asr_gru_workspace_bytes(T, B, H))


def device_lengths(lengths: Sequence[int]) -> DeviceBytes:
    """Utterance lengths as the device int32 [B] array asr_lstm_* read."""
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    d = DeviceBytes(max(ln.nbytes, 4))
    check(lib().asr_memcpy_h2d(d.ptr, _ptr(ln), ln.nbytes, None), "asr_memcpy_h2d")
    return d


def _gated_tail(kind: str, hid: DeviceMatrix, col: int, H: int, T: int, B: int, work, need_work: bool, *optional):
    """Arguments shared by lstm_fwd / lstm_recur_fwd / gru_fwd / gru_recur_fwd
    (kind "LSTM" or "GRU"): the output pointer of the direction that writes
    columns [col, col + H) of hid's rows, its row stride, and the pointers of
    the optional buffers (None stays None).  need_work: the call needs the
    whole asr_<kind>_workspace_bytes in work."""
    assert hid.rows == T * B and 0 <= col and col + H <= hid.cols, (hid.rows, hid.cols, col, H)
    if need_work:
        name = f"asr_{kind.lower()}_workspace_bytes"
        need = int(getattr(lib(), name)(T, B, H))
        if need and (work is None or work.nbytes < need):
            raise ValueError(f"{kind} workspace of {need} bytes needed ({name})")
    return (hid.ptr + 4 * col, hid.cols) + tuple(m.ptr if m is not None else None for m in optional)


def lstm_fwd(x: DeviceMatrix, W_ih: DeviceMatrix, W_hh: DeviceMatrix, b_ih: DeviceMatrix, b_hh: DeviceMatrix,
             hid: DeviceMatrix, T: int, B: int, work: DeviceBytes, h0: Optional[DeviceMatrix] = None,
             c0: Optional[DeviceMatrix] = None, hT: Optional[DeviceMatrix] = None,
             cT: Optional[DeviceMatrix] = None, lengths: Optional[DeviceBytes] = None, reverse: bool = False,
             col: int = 0, stream: int = 0) -> DeviceMatrix:
    """One LSTM layer and direction (asr_lstm_fwd): W_ih [in, 4H], W_hh [H, 4H]
    (gates i, f, g, o), h_t into columns [col, col + H) of hid [T*B, >= H]
    (the row stride is hid.cols); lengths from device_lengths().  hT may be h0
    itself (in-place streaming) for H <= 128 only: for H > 128, and for any
    partial overlap of the two, the library returns ASR_ERR_ARG (asr_amd.h);
    cT may be c0."""
    inp, H = W_ih.rows, W_hh.rows
    assert x.rows == T * B and x.cols == inp and W_ih.cols == 4 * H and W_hh.cols == 4 * H
    out, ldh, pht, pct, pln, pwk = _gated_tail("LSTM", hid, col, H, T, B, work, True, hT, cT, lengths, work)
    check(lib().asr_lstm_fwd(x.ptr, h0.ptr if h0 else None, c0.ptr if c0 else None, W_ih.ptr, W_hh.ptr,
                             b_ih.ptr, b_hh.ptr, out, ldh, pht, pct, pln, pwk, T, B, inp, H,
                             int(bool(reverse)), stream), "asr_lstm_fwd")
    return hid


def lstm_recur_fwd(P: DeviceMatrix, W_hh: DeviceMatrix, b_ih: DeviceMatrix, b_hh: DeviceMatrix,
                   hid: DeviceMatrix, T: int, B: int, work: Optional[DeviceBytes] = None,
                   h0: Optional[DeviceMatrix] = None, c0: Optional[DeviceMatrix] = None,
                   hT: Optional[DeviceMatrix] = None, cT: Optional[DeviceMatrix] = None,
                   lengths: Optional[DeviceBytes] = None, reverse: bool = False, col: int = 0,
                   stream: int = 0) -> DeviceMatrix:
    """The recurrence stage alone (asr_lstm_recur_fwd): P [T*B, 4H] holds x.W_ih
    (read only); work is needed for H > 128.  hT may be h0 itself (in-place
    streaming) for H <= 128 only: for H > 128, and for any partial overlap of
    the two, the library returns ASR_ERR_ARG (asr_amd.h); cT may be c0."""
    H = W_hh.rows
    assert P.rows == T * B and P.cols == 4 * H and W_hh.cols == 4 * H
    out, ldh, pht, pct, pln, pwk = _gated_tail("LSTM", hid, col, H, T, B, work, H > 128, hT, cT, lengths, work)
    check(lib().asr_lstm_recur_fwd(P.ptr, h0.ptr if h0 else None, c0.ptr if c0 else None, W_hh.ptr, b_ih.ptr,
                                   b_hh.ptr, out, ldh, pht, pct, pln, pwk, T, B, H, int(bool(reverse)),
                                   stream), "asr_lstm_recur_fwd")
    return hid


def gru_fwd(x: DeviceMatrix, W_ih: DeviceMatrix, W_hh: DeviceMatrix, b_ih: DeviceMatrix, b_hh: DeviceMatrix,
            hid: DeviceMatrix, T: int, B: int, work: DeviceBytes, h0: Optional[DeviceMatrix] = None,
            hT: Optional[DeviceMatrix] = None, lengths: Optional[DeviceBytes] = None, reverse: bool = False,
            col: int = 0, stream: int = 0) -> DeviceMatrix:
    """One GRU layer and direction (asr_gru_fwd): W_ih [in, 3H], W_hh [H, 3H]
    (gates r, z, n), h_t into columns [col, col + H) of hid [T*B, >= H] (the
    row stride is hid.cols); lengths from device_lengths().  hT may be h0
    itself (in-place streaming) for H <= 128 only: for H > 128, and for any
    partial overlap of the two, the library returns ASR_ERR_ARG (asr_amd.h)."""
    inp, H = W_ih.rows, W_hh.rows
    assert x.rows == T * B and x.cols == inp and W_ih.cols == 3 * H and W_hh.cols == 3 * H
    out, ldh, pht, pln, pwk = _gated_tail("GRU", hid, col, H, T, B, work, True, hT, lengths, work)
    check(lib().asr_gru_fwd(x.ptr, h0.ptr if h0 else None, W_ih.ptr, W_hh.ptr, b_ih.ptr, b_hh.ptr, out, ldh, pht,
                            pln, pwk, T, B, inp, H, int(bool(reverse)), stream), "asr_gru_fwd")
    return hid


def gru_recur_fwd(P: DeviceMatrix, W_hh: DeviceMatrix, b_ih: DeviceMatrix, b_hh: DeviceMatrix, hid: DeviceMatrix,
                  T: int, B: int, h0: Optional[DeviceMatrix] = None, hT: Optional[DeviceMatrix] = None,
                  lengths: Optional[DeviceBytes] = None, reverse: bool = False, col: int = 0,
                  stream: int = 0) -> DeviceMatrix:
    """The recurrence stage alone (asr_gru_recur_fwd): P [T*B, 3H] holds x.W_ih
    (read only); no workspace.  hT may be h0 itself (in-place streaming) for
    H <= 128 only: for H > 128, and for any partial overlap of the two, the
    library returns ASR_ERR_ARG (asr_amd.h)."""
    H = W_hh.rows
    assert P.rows == T * B and P.cols == 3 * H and W_hh.cols == 3 * H
    out, ldh, pht, pln = _gated_tail("GRU", hid, col, H, T, B, None, False, hT, lengths)
    check(lib().asr_gru_recur_fwd(P.ptr, h0.ptr if h0 else None, W_hh.ptr, b_ih.ptr, b_hh.ptr, out, ldh, pht, pln,
                                  T, B, H, int(bool(reverse)), stream), "asr_gru_recur_fwd")
    return hid


class _DeviceView:
    """Rows [r0, r0 + rows) of a DeviceMatrix, without owning them."""

    def __init__(self, m: DeviceMatrix, r0: int, rows: int):
        self.ptr, self.rows, self.cols, self._keep = m.ptr + 4 * r0 * m.cols, rows, m.cols, m


class _GatedRNN:
    """What LSTM and GRU share: the device weights of every layer and direction,
    one workspace, from_torch and the layer / direction loop of forward.  A
    subclass names its gate count (_NG), its state matrices (_STATES, h_n
    first), its workspace function, what from_torch refuses and the call of one
    layer and direction."""
    _NG = 0
    _STATES: Tuple[str, ...] = ()

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1, bidirectional: bool = False,
                 params: Optional[Sequence[Sequence[Tuple[np.ndarray, ...]]]] = None):
        self.inp, self.H, self.L, self.D = input_size, hidden_size, num_layers, 2 if bidirectional else 1
        H, G = hidden_size, self._NG * hidden_size
        self.layers = []
        for l in range(num_layers):
            i = input_size if l == 0 else self.D * H
            shapes = ((i, G), (H, G), (G, 1), (G, 1))
            dirs = []
            for d in range(self.D):
                p = [np.zeros(s, np.float32) for s in shapes] if params is None else params[l][d]
                dirs.append(tuple(DeviceMatrix.from_numpy(np.asarray(a, np.float32).reshape(s))
                                  for a, s in zip(p, shapes)))
            self.layers.append(dirs)
        self._work: Optional[DeviceBytes] = None
        self._shape = None
        self.outputs: List[DeviceMatrix] = []
        for name in self._STATES:   # each [L*D*B, H] as torch's h_n [L*D, B, H]
            setattr(self, name, None)

    @classmethod
    def from_torch(cls, module):
        """The weight_*_l{k}[_reverse] tensors of the torch.nn module of the same
        name, transposed to [in][out], and its biases."""
        cls._refuse(module)
        params = []
        for l in range(module.num_layers):
            dirs = []
            for sfx in ("", "_reverse")[:2 if module.bidirectional else 1]:
                get = lambda n: getattr(module, f"{n}_l{l}{sfx}").detach().cpu().float().numpy()   # noqa: E731
                dirs.append((np.ascontiguousarray(get("weight_ih").T), np.ascontiguousarray(get("weight_hh").T),
                             get("bias_ih"), get("bias_hh")))
            params.append(dirs)
        return cls(module.input_size, module.hidden_size, module.num_layers, module.bidirectional, params)

    def _forward(self, x: DeviceMatrix, T: int, B: int, lengths, h0: Optional[DeviceMatrix], st: int) -> DeviceMatrix:
        """The layers in turn, the two directions of a layer into the two halves
        of one buffer; state k of _layer is rows [k, k + B) of h_n (c_n, h0)."""
        H, D = self.H, self.D
        if self._shape != (T, B):
            need = self._workspace_bytes(T, B, H)
            if not need:
                raise AsrError(ASR_ERR_UNSUPPORTED, f"asr_{type(self).__name__.lower()}_workspace_bytes")
            if self._work is None or self._work.nbytes < need:
                self._work = DeviceBytes(need)
            self.outputs = [DeviceMatrix(T * B, D * H) for _ in range(self.L)]
            for name in self._STATES:
                setattr(self, name, DeviceMatrix(self.L * D * B, H))
            self._shape = (T, B)
        assert h0 is None or (h0.rows == self.L * D * B and h0.cols == H), (h0.rows, h0.cols)
        if h0 is not None and h0.ptr < self.h_n.ptr + self.h_n.nbytes and self.h_n.ptr < h0.ptr + h0.nbytes:
            # h0 is (part of) the state matrix about to be written, e.g. h0=net.h_n: the step form cannot
            # write d_hT over d_h0 (asr_amd.h), so the new state goes to a second matrix; no device copy,
            # and the caller's h0 keeps its contents
            self.h_n = DeviceMatrix(self.L * D * B, H)
        ln = lengths if lengths is None or isinstance(lengths, DeviceBytes) else device_lengths(lengths)
        for l, dirs in enumerate(self.layers):
            for d, weights in enumerate(dirs):
                self._layer(x, weights, self.outputs[l], T, B, (l * D + d) * B, h0, lengths=ln, reverse=d == 1,
                            col=d * H, stream=st)
            x = self.outputs[l]
        if ln is not None:   # the kernels read it: keep it until they are done
            check(lib().asr_stream_sync(ctypes.c_void_p(st or None)), "asr_stream_sync")
        return self.outputs[-1]


class LSTM(_GatedRNN):
    """torch.nn.LSTM(input_size, hidden_size, num_layers, bidirectional=...) for
    inference on asr_lstm_fwd: device weights and one workspace, no arithmetic
    here.  params[layer][direction] = (W_ih [in, 4H], W_hh [H, 4H], b_ih [4H],
    b_hh [4H]) in this library's [in][out] layout (zeros if None); from_torch
    takes them from a torch module.  No proj_size, no dropout."""
    _NG, _STATES = 4, ("h_n", "c_n")
    _workspace_bytes = staticmethod(lstm_workspace_bytes)

    @staticmethod
    def _refuse(module) -> None:
        if getattr(module, "proj_size", 0) or not module.bias:
            raise ValueError("LSTM.from_torch: proj_size and bias=False are not supported")

    def _layer(self, x, weights, out, T, B, k, h0, **kw) -> None:
        lstm_fwd(x, *weights, out, T, B, self._work, hT=_DeviceView(self.h_n, k, B), cT=_DeviceView(self.c_n, k, B),
                 **kw)

    def forward(self, x: DeviceMatrix, T: int, B: int, lengths: Optional[Sequence[int]] = None,
                stream: Optional[int] = None) -> DeviceMatrix:
        """x time-major [T*B, input_size]; lengths: a sequence of B counts or a
        device int32 [B] (DeviceBytes, e.g. Conv1d.forward's out_lengths);
        returns the last layer's [T*B, H or 2H] (zeros past each utterance's
        length); h_n / c_n hold the final states.  The two directions of a layer
        write the two halves of one buffer."""
        return self._forward(x, T, B, lengths, None, stream or 0)


class GRU(_GatedRNN):
    """torch.nn.GRU(input_size, hidden_size, num_layers, bidirectional=...) for
    inference on asr_gru_fwd: device weights and one workspace, no arithmetic
    here.  params[layer][direction] = (W_ih [in, 3H], W_hh [H, 3H], b_ih [3H],
    b_hh [3H]) in this library's [in][out] layout (zeros if None); from_torch
    takes them from a torch module.  No dropout."""
    _NG, _STATES = 3, ("h_n",)
    _workspace_bytes = staticmethod(gru_workspace_bytes)

    @staticmethod
    def _refuse(module) -> None:
        if not module.bias:
            raise ValueError("GRU.from_torch: bias=False is not supported")

    def _layer(self, x, weights, out, T, B, k, h0, **kw) -> None:
        gru_fwd(x, *weights, out, T, B, self._work, h0=None if h0 is None else _DeviceView(h0, k, B),
                hT=_DeviceView(self.h_n, k, B), **kw)

    def forward(self, x: DeviceMatrix, T: int, B: int, lengths: Optional[Sequence[int]] = None,
                h0: Optional[DeviceMatrix] = None, stream: Optional[int] = None) -> DeviceMatrix:
        """x time-major [T*B, input_size]; h0 [L*D*B, H] in h_n's order (None =
        zeros); lengths: a sequence of B counts or a device int32 [B]
        (DeviceBytes, e.g. Conv1d.forward's out_lengths); returns the last
        layer's [T*B, H or 2H] (zeros past each utterance's length); h_n holds
        the final states.  The two directions of a layer write the two halves
        of one buffer.  h0=net.h_n streams: the kernels cannot write the new
        state over the one they read for H > 128 (asr_amd.h), so when h0 shares
        memory with h_n the new state is written to a second matrix, which
        becomes h_n; the caller's h0 keeps its contents and nothing is copied."""
        return self._forward(x, T, B, lengths, h0, stream or 0)


# -------------------------------------------------------------------- Conv1d
CONV_ACT_NONE, CONV_ACT_RELU, CONV_ACT_CLIP = 0, 1, 2
CONV_ACTS = {None: CONV_ACT_NONE, "none": CONV_ACT_NONE, "relu": CONV_ACT_RELU, "clip": CONV_ACT_CLIP}


class Conv1dDesc(ctypes.Structure):
    """asr_conv1d_desc (include/asr_amd.h)."""
    _fields_ = [("c_in", _i), ("c_out", _i), ("kernel", _i), ("stride", _i), ("dilation", _i),
                ("pad_left", _i), ("pad_right", _i), ("groups", _i), ("act", _i), ("clip", _f)]


def conv1d_desc(c_in: int, c_out: int, kernel: int, stride: int = 1, dilation: int = 1, pad_left: int = 0,
                pad_right: int = 0, groups: int = 1, act=None, clip: float = 20.0) -> Conv1dDesc:
    """A Conv1dDesc from keywords; act: None, "relu", "clip" or an ASR_CONV_ACT_* value."""
    a = CONV_ACTS[act.lower()] if isinstance(act, str) else CONV_ACT_NONE if act is None else int(act)
    return Conv1dDesc(c_in, c_out, kernel, stride, dilation, pad_left, pad_right, groups, a, clip)


def conv1d_out_frames(desc, n: int) -> int:
    """asr_conv1d_out_frames: frames out for n frames in (< 0 for a bad
    descriptor); desc is a Conv1dDesc or the keywords of conv1d_desc."""
    d = desc if isinstance(desc, Conv1dDesc) else conv1d_desc(**desc)
    return int(lib().asr_conv1d_out_frames(ctypes.byref(d), int(n)))


def conv1d_fwd(x: DeviceMatrix, W: DeviceMatrix, b: Optional[DeviceMatrix], out: DeviceMatrix, T: int, B: int,
               desc: Conv1dDesc, lengths: Optional[DeviceBytes] = None, out_lengths: Optional[DeviceBytes] = None,
               col: int = 0, stream: int = 0) -> DeviceMatrix:
    """One convolution over time (asr_conv1d_fwd): x [T*B, >= c_in] time-major
    (the row stride is x.cols), W [k * c_in / groups, c_out], b [c_out] or None,
    the result into columns [col, col + c_out) of out [T_out*B, >= c_out] (the
    row stride is out.cols); lengths from device_lengths(), out_lengths a
    DeviceBytes of 4*B bytes."""
    T_out = conv1d_out_frames(desc, T)
    assert x.rows == T * B and x.cols >= desc.c_in, (x.rows, x.cols)
    assert T_out <= 0 or out.rows == T_out * B, (out.rows, T_out, B)
    assert 0 <= col and col + desc.c_out <= out.cols, (out.cols, col)
    assert W.rows * W.cols == desc.kernel * (desc.c_in // max(desc.groups, 1)) * desc.c_out, (W.rows, W.cols)
    assert out_lengths is None or out_lengths.nbytes >= 4 * B
    opt = lambda m: m.ptr if m is not None else None   # noqa: E731
    check(lib().asr_conv1d_fwd(ctypes.byref(desc), x.ptr, x.cols, opt(lengths), W.ptr, opt(b), out.ptr + 4 * col,
                               out.cols, opt(out_lengths), T, B, stream), "asr_conv1d_fwd")
    return out


class Conv1d:
    """torch.nn.Conv1d(c_in, c_out, kernel, stride, dilation=..., groups=...)
    over time for inference on asr_conv1d_fwd, time-major in and out, bias and
    activation fused; no arithmetic here.  padding: an int (both sides),
    (left, right), 'valid', 'same' (stride 1 only; left = total // 2, right =
    total - left, as torch) or 'causal' (left = dilation * (kernel - 1));
    groups 1 or c_in == c_out == groups; act None, 'relu' or 'clip'
    (min(max(v, 0), clip)); weight [k][c_in / groups][c_out] and bias [c_out]
    in this library's layout (zeros if None; pack_torch makes them from a torch
    module)."""

    def __init__(self, c_in: int, c_out: int, kernel: int, stride: int = 1, dilation: int = 1, padding=0,
                 groups: int = 1, act=None, clip: float = 20.0, weight=None, bias=None):
        pl, pr = self.parse_padding(padding, kernel, stride, dilation)
        self.desc = conv1d_desc(c_in, c_out, kernel, stride, dilation, pl, pr, groups, act, clip)
        rc = conv1d_out_frames(self.desc, 1)
        if rc < 0:
            raise AsrError(-rc, "asr_conv1d_out_frames")
        shape = (kernel * (c_in // groups), c_out)
        w = np.zeros(shape, np.float32) if weight is None else np.asarray(weight, np.float32).reshape(shape)
        b = np.zeros(c_out, np.float32) if bias is None else np.asarray(bias, np.float32).reshape(c_out)
        self.W, self.b = DeviceMatrix.from_numpy(w), DeviceMatrix.from_numpy(b.reshape(-1, 1))
        self._keep = None   # the last call's uploaded lengths: alive until its kernel is done

    @staticmethod
    def parse_padding(padding, kernel: int, stride: int = 1, dilation: int = 1) -> Tuple[int, int]:
        """(pad_left, pad_right) of a padding argument."""
        total = dilation * (kernel - 1)
        if isinstance(padding, str):
            if padding == "valid":
                return 0, 0
            if padding == "causal":
                return total, 0
            if padding == "same":
                if stride != 1:
                    raise ValueError("Conv1d: padding='same' takes stride 1 only")
                return total // 2, total - total // 2
            raise ValueError(f"Conv1d: unknown padding {padding!r}")
        if isinstance(padding, (tuple, list)):
            if len(padding) == 1:
                return int(padding[0]), int(padding[0])
            if len(padding) != 2:
                raise ValueError(f"Conv1d: padding {padding!r}")
            return int(padding[0]), int(padding[1])
        return int(padding), int(padding)

    @staticmethod
    def pack_torch(conv, bn=None):
        """(W [k][c_in/g][c_out] float32, b [c_out] float32, keywords of Conv1d)
        from a torch.nn.Conv1d; with bn an eval-mode torch.nn.BatchNorm1d is
        folded in float64 (W' = W g / sqrt(var + eps) per output channel,
        b' = (b - mean) g / sqrt(var + eps) + beta) and the result rounded to
        fp32 once.  No device call."""
        if conv.padding_mode != "zeros":
            raise ValueError(f"Conv1d.pack_torch: padding_mode {conv.padding_mode!r} is not supported")
        c_in, c_out, g = conv.in_channels, conv.out_channels, conv.groups
        if g != 1 and not (g == c_in == c_out):
            raise ValueError("Conv1d.pack_torch: groups must be 1 or c_in == c_out == groups")
        k, s, d = conv.kernel_size[0], conv.stride[0], conv.dilation[0]
        w = conv.weight.detach().cpu().double().numpy()                  # [c_out][c_in/g][k]
        b = (conv.bias.detach().cpu().double().numpy() if conv.bias is not None else np.zeros(c_out, np.float64))
        if bn is not None:
            if bn.training or bn.running_mean is None or bn.running_var is None:
                raise ValueError("Conv1d.pack_torch: the BatchNorm1d must be in eval() with running statistics")
            if bn.num_features != c_out:
                raise ValueError("Conv1d.pack_torch: BatchNorm1d features != c_out")
            mean = bn.running_mean.detach().cpu().double().numpy()
            var = bn.running_var.detach().cpu().double().numpy()
            gamma = bn.weight.detach().cpu().double().numpy() if bn.affine else np.ones(c_out)
            beta = bn.bias.detach().cpu().double().numpy() if bn.affine else np.zeros(c_out)
            scale = gamma / np.sqrt(var + bn.eps)
            w = w * scale[:, None, None]
            b = (b - mean) * scale + beta
        W = np.ascontiguousarray(w.transpose(2, 1, 0)).astype(np.float32)   # [k][c_in/g][c_out]
        pad = conv.padding if isinstance(conv.padding, str) else tuple(int(v) for v in conv.padding)
        pl, pr = Conv1d.parse_padding(pad, k, s, d)
        kwargs = dict(c_in=c_in, c_out=c_out, kernel=k, stride=s, dilation=d, padding=(pl, pr), groups=g)
        return W, b.astype(np.float32), kwargs

    @classmethod
    def from_torch(cls, conv, bn=None, act=None, clip: float = 20.0) -> "Conv1d":
        W, b, kw = cls.pack_torch(conv, bn)
        return cls(**kw, act=act, clip=clip, weight=W, bias=b)

    def out_frames(self, n: int) -> int:
        return conv1d_out_frames(self.desc, n)

    def forward(self, x: DeviceMatrix, T: int, B: int, lengths=None, stream: int = 0):
        """x time-major [T*B, c_in]; lengths None, a sequence of B counts or a
        DeviceBytes of int32 [B].  Returns (out DeviceMatrix [T_out*B, c_out]
        with zero rows past each utterance's count, T_out, out_lengths): the
        last a DeviceBytes of int32 [B] that GRU.forward / LSTM.forward take as
        lengths, or None when no lengths were given.  Asynchronous on stream."""
        T_out = self.out_frames(T)
        if T_out <= 0:
            raise AsrError(ASR_ERR_ARG if T_out == 0 else -T_out, "asr_conv1d_out_frames")
        if lengths is not None and not isinstance(lengths, DeviceBytes):
            lengths = device_lengths(lengths)
        out = DeviceMatrix(T_out * B, self.desc.c_out)
        oln = None if lengths is None else DeviceBytes(4 * B)
        conv1d_fwd(x, self.W, self.b, out, T, B, self.desc, lengths=lengths, out_lengths=oln, stream=stream or 0)
        self._keep = lengths
        return out, T_out, oln


# -------------------------------------------------------------------- Conv2d
class Conv2dDesc(ctypes.Structure):
    """asr_conv2d_desc (include/asr_amd.h)."""
    _fields_ = [("c_in", _i), ("c_out", _i), ("feat_in", _i), ("kernel_t", _i), ("kernel_f", _i),
                ("stride_t", _i), ("stride_f", _i), ("pad_t_lo", _i), ("pad_t_hi", _i), ("pad_f_lo", _i),
                ("pad_f_hi", _i), ("groups", _i), ("act", _i), ("clip", _f)]


def conv2d_desc(c_in: int, c_out: int, feat_in: int, kernel_t: int, kernel_f: int, stride_t: int = 1,
                stride_f: int = 1, pad_t_lo: int = 0, pad_t_hi: int = 0, pad_f_lo: int = 0, pad_f_hi: int = 0,
                groups: int = 1, act=None, clip: float = 20.0) -> Conv2dDesc:
    """A Conv2dDesc from keywords; act: None, "relu", "clip" or an ASR_CONV_ACT_* value."""
    a = CONV_ACTS[act.lower()] if isinstance(act, str) else CONV_ACT_NONE if act is None else int(act)
    return Conv2dDesc(c_in, c_out, feat_in, kernel_t, kernel_f, stride_t, stride_f, pad_t_lo, pad_t_hi, pad_f_lo,
                      pad_f_hi, groups, a, clip)


def conv2d_out_frames(desc, n: int) -> int:
    """asr_conv2d_out_frames: frames out for n frames in (< 0 for a bad
    descriptor); desc is a Conv2dDesc or the keywords of conv2d_desc."""
    d = desc if isinstance(desc, Conv2dDesc) else conv2d_desc(**desc)
    return int(lib().asr_conv2d_out_frames(ctypes.byref(d), int(n)))


def conv2d_out_feats(desc) -> int:
    """asr_conv2d_out_feats: frequency bins out, F_out >= 1 (< 0 for a bad
    descriptor); desc is a Conv2dDesc or the keywords of conv2d_desc."""
    d = desc if isinstance(desc, Conv2dDesc) else conv2d_desc(**desc)
    return int(lib().asr_conv2d_out_feats(ctypes.byref(d)))


def conv2d_fwd(x: DeviceMatrix, W: DeviceMatrix, b: Optional[DeviceMatrix], out: DeviceMatrix, T: int, B: int,
               desc: Conv2dDesc, lengths: Optional[DeviceBytes] = None, out_lengths: Optional[DeviceBytes] = None,
               col: int = 0, stream: int = 0) -> DeviceMatrix:
    """One convolution over (time, frequency) (asr_conv2d_fwd): x [T*B, >=
    feat_in * c_in] time-major, element (f, ci) of a row at f * c_in + ci (the
    row stride is x.cols), W [kernel_t * kernel_f * c_in / groups, c_out], b
    [c_out] or None, the result into columns [col, col + F_out * c_out) of out
    [T_out*B, ...] (the row stride is out.cols); lengths from device_lengths(),
    out_lengths a DeviceBytes of 4*B bytes."""
    T_out, F_out = conv2d_out_frames(desc, T), conv2d_out_feats(desc)
    assert x.rows == T * B and x.cols >= desc.feat_in * desc.c_in, (x.rows, x.cols)
    assert T_out <= 0 or out.rows == T_out * B, (out.rows, T_out, B)
    assert F_out <= 0 or (0 <= col and col + F_out * desc.c_out <= out.cols), (out.cols, col, F_out)
    assert W.rows * W.cols == desc.kernel_t * desc.kernel_f * (desc.c_in // max(desc.groups, 1)) * desc.c_out, \
        (W.rows, W.cols)
    assert out_lengths is None or out_lengths.nbytes >= 4 * B
    opt = lambda m: m.ptr if m is not None else None   # noqa: E731
    check(lib().asr_conv2d_fwd(ctypes.byref(desc), x.ptr, x.cols, opt(lengths), W.ptr, opt(b), out.ptr + 4 * col,
                               out.cols, opt(out_lengths), T, B, stream), "asr_conv2d_fwd")
    return out


def _pair(v, what: str) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"Conv2d: {what} {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


class Conv2d:
    """torch.nn.Conv2d(c_in, c_out, kernel, stride, groups=...) on an input
    [B][C][T][F] for inference on asr_conv2d_fwd, time-major in and out (row
    t*B + b holds F * c_in floats, element (f, ci) at f * c_in + ci), bias and
    activation fused; no arithmetic here.  kernel, stride: an int or (time,
    frequency); padding: an int, torch's (time, frequency) (both sides of each
    axis), 'valid', or ((t_lo, t_hi), (f_lo, f_hi)); groups 1 or c_in == c_out
    == groups; act None, 'relu' or 'clip'; weight [kt][kf][c_in / groups][c_out]
    and bias [c_out] in this library's layout (zeros if None; pack_torch makes
    them from a torch module)."""

    def __init__(self, c_in: int, c_out: int, feat_in: int, kernel, stride=1, padding=0, groups: int = 1, act=None,
                 clip: float = 20.0, weight=None, bias=None):
        self.desc = self.make_desc(c_in, c_out, feat_in, kernel, stride, padding, groups, act, clip)
        kt, kf = self.desc.kernel_t, self.desc.kernel_f
        rc = conv2d_out_feats(self.desc)
        if rc < 0:
            raise AsrError(-rc, "asr_conv2d_out_feats")
        self.feat_out = rc
        shape = (kt * kf * (c_in // groups), c_out)
        w = np.zeros(shape, np.float32) if weight is None else np.asarray(weight, np.float32).reshape(shape)
        b = np.zeros(c_out, np.float32) if bias is None else np.asarray(bias, np.float32).reshape(c_out)
        self.W, self.b = DeviceMatrix.from_numpy(w), DeviceMatrix.from_numpy(b.reshape(-1, 1))
        self._keep = None   # the last call's uploaded lengths: alive until its kernel is done

    @staticmethod
    def make_desc(c_in: int, c_out: int, feat_in: int, kernel, stride=1, padding=0, groups: int = 1, act=None,
                  clip: float = 20.0) -> Conv2dDesc:
        """The Conv2dDesc of the constructor's keywords.  No device call."""
        (kt, kf), (st, sf) = _pair(kernel, "kernel"), _pair(stride, "stride")
        (ptl, pth), (pfl, pfh) = Conv2d.parse_padding(padding)
        return conv2d_desc(c_in, c_out, feat_in, kt, kf, st, sf, ptl, pth, pfl, pfh, groups, act, clip)

    @staticmethod
    def parse_padding(padding) -> Tuple[Tuple[int, int], Tuple[int, int]]:
        """((pad_t_lo, pad_t_hi), (pad_f_lo, pad_f_hi)) of a padding argument."""
        if isinstance(padding, str):
            if padding == "valid":
                return (0, 0), (0, 0)
            raise ValueError(f"Conv2d: padding {padding!r} is not supported")
        if isinstance(padding, (tuple, list)):
            if len(padding) != 2:
                raise ValueError(f"Conv2d: padding {padding!r}")
            if isinstance(padding[0], (tuple, list)) or isinstance(padding[1], (tuple, list)):
                return _pair(padding[0], "padding"), _pair(padding[1], "padding")
            return (int(padding[0]),) * 2, (int(padding[1]),) * 2
        return (int(padding),) * 2, (int(padding),) * 2

    @staticmethod
    def pack_torch(conv, bn=None):
        """(W [kt][kf][c_in/g][c_out] float32, b [c_out] float32, keywords of
        Conv2d without feat_in) from a torch.nn.Conv2d whose input is
        [B][C][T][F]; with bn an eval-mode torch.nn.BatchNorm2d is folded in
        float64 (W' = W g / sqrt(var + eps) per output channel, b' = (b - mean) g
        / sqrt(var + eps) + beta) and the result rounded to fp32 once.  No
        device call."""
        if conv.padding_mode != "zeros":
            raise ValueError(f"Conv2d.pack_torch: padding_mode {conv.padding_mode!r} is not supported")
        if tuple(conv.dilation) != (1, 1):
            raise ValueError(f"Conv2d.pack_torch: dilation {tuple(conv.dilation)} is not supported")
        c_in, c_out, g = conv.in_channels, conv.out_channels, conv.groups
        if g != 1 and not (g == c_in == c_out):
            raise ValueError("Conv2d.pack_torch: groups must be 1 or c_in == c_out == groups")
        w = conv.weight.detach().cpu().double().numpy()                  # [c_out][c_in/g][kt][kf]
        b = (conv.bias.detach().cpu().double().numpy() if conv.bias is not None else np.zeros(c_out, np.float64))
        if bn is not None:
            if bn.training or bn.running_mean is None or bn.running_var is None:
                raise ValueError("Conv2d.pack_torch: the BatchNorm2d must be in eval() with running statistics")
            if bn.num_features != c_out:
                raise ValueError("Conv2d.pack_torch: BatchNorm2d features != c_out")
            mean = bn.running_mean.detach().cpu().double().numpy()
            var = bn.running_var.detach().cpu().double().numpy()
            gamma = bn.weight.detach().cpu().double().numpy() if bn.affine else np.ones(c_out)
            beta = bn.bias.detach().cpu().double().numpy() if bn.affine else np.zeros(c_out)
            scale = gamma / np.sqrt(var + bn.eps)
            w = w * scale[:, None, None, None]
            b = (b - mean) * scale + beta
        W = np.ascontiguousarray(w.transpose(2, 3, 1, 0)).astype(np.float32)   # [kt][kf][c_in/g][c_out]
        pad = conv.padding if isinstance(conv.padding, str) else tuple(int(v) for v in conv.padding)
        kwargs = dict(c_in=c_in, c_out=c_out, kernel=tuple(int(v) for v in conv.kernel_size),
                      stride=tuple(int(v) for v in conv.stride), padding=Conv2d.parse_padding(pad), groups=g)
        return W, b.astype(np.float32), kwargs

    @classmethod
    def from_torch(cls, conv, bn=None, act=None, clip: float = 20.0, *, feat_in: int) -> "Conv2d":
        """feat_in: the frequency bins F of the input (a torch.nn.Conv2d does not know them)."""
        W, b, kw = cls.pack_torch(conv, bn)
        return cls(feat_in=feat_in, **kw, act=act, clip=clip, weight=W, bias=b)

    def out_frames(self, n: int) -> int:
        return conv2d_out_frames(self.desc, n)

    def forward(self, x: DeviceMatrix, T: int, B: int, lengths=None, stream: int = 0):
        """x time-major [T*B, >= feat_in * c_in]; lengths None, a sequence of B
        counts or a DeviceBytes of int32 [B].  Returns (out DeviceMatrix
        [T_out*B, F_out * c_out] with zero rows past each utterance's count,
        T_out, out_lengths): the last a DeviceBytes of int32 [B] that the next
        layer takes as lengths, or None when no lengths were given.
        Asynchronous on stream."""
        T_out = self.out_frames(T)
        if T_out <= 0:
            raise AsrError(ASR_ERR_ARG if T_out == 0 else -T_out, "asr_conv2d_out_frames")
        lengths = _device_lengths_or_none(lengths)
        out = DeviceMatrix(T_out * B, self.feat_out * self.desc.c_out)
        oln = None if lengths is None else DeviceBytes(4 * B)
        conv2d_fwd(x, self.W, self.b, out, T, B, self.desc, lengths=lengths, out_lengths=oln, stream=stream or 0)
        self._keep = lengths
        return out, T_out, oln


class Conv2dSubsampling:
    """The module Conformer encoders of ESPnet / WeNet (Conv2dSubsampling4 / 6 /
    8: .conv, .out[0]) and NeMo (ConvSubsampling 'striding' / 'dw_striding':
    .conv, .out) begin with, for inference, time-major: strided Conv2d layers
    over (time, frequency) with their ReLUs fused (asr_conv2d_fwd, the
    out_lengths of each the lengths of the next), then the Linear over the
    flattened (channel, frequency) axis (asr_linear_fwd with EPI_BIAS), then
    asr_mask_rows.  No arithmetic here.  The Linear's input rows are permuted
    when packing from the toolkits' c * F' + f order to this library's f * C +
    c, and scale (the toolkits' xscale = sqrt(E), applied after the module) is
    folded into its weights and bias in float64 before the one rounding to fp32.
    Tested on stand-in modules written from the toolkits' published
    definitions only (tests/conv2d_reference.py), never on the toolkits
    themselves or their checkpoints."""

    def __init__(self, layers: Sequence[Conv2d], w_out, b_out):
        self.layers = list(layers)
        assert self.layers
        for a, b in zip(self.layers, self.layers[1:]):
            assert b.desc.c_in == a.desc.c_out and b.desc.feat_in == a.feat_out, "the layers do not chain"
        self.feat_in, self.c_in = self.layers[0].desc.feat_in, self.layers[0].desc.c_in
        last = self.layers[-1]
        w = np.asarray(w_out, np.float32)
        assert w.ndim == 2 and w.shape[0] == last.feat_out * last.desc.c_out, w.shape
        self.E = w.shape[1]
        self.w_out = DeviceMatrix.from_numpy(w)
        self.b_out = DeviceMatrix.from_numpy(np.asarray(b_out, np.float32).reshape(self.E, 1))
        self._scratch, self._keep = _Scratch(), None

    @staticmethod
    def pack_linear(out, c_out: int, feat_out: int, scale: float = 1.0):
        """(W [feat_out * c_out, E], b [E]) float32 of the module's Linear: row
        f * c_out + c of W is column c * feat_out + f of out.weight, both times
        scale in float64, rounded once.  No device call."""
        if out.in_features != c_out * feat_out:
            raise ValueError(f"Conv2dSubsampling: the Linear takes {out.in_features} inputs, the convolutions make "
                             f"{c_out} channels x {feat_out} bins")
        w = out.weight.detach().cpu().double().numpy() * float(scale)              # [E][c * F' + f]
        b = (out.bias.detach().cpu().double().numpy() if out.bias is not None
             else np.zeros(out.out_features)) * float(scale)
        E = out.out_features
        w = w.reshape(E, c_out, feat_out).transpose(2, 1, 0).reshape(feat_out * c_out, E)
        return np.ascontiguousarray(w).astype(np.float32), b.astype(np.float32)

    @staticmethod
    def pack_torch(conv, out, feat_in: int, scale: float = 1.0, causal: bool = False):
        """(layers, w_out, b_out) on the host: layers a list of the keywords of
        Conv2d (feat_in, act, weight and bias included) of every Conv2d of the
        Sequential, w_out / b_out as pack_linear makes them.  The arguments are
        from_torch's; every refusal is decided here.  No device call."""
        import torch
        mods, layers, F = list(conv), [], int(feat_in)
        i = 0
        while i < len(mods):
            m = mods[i]
            if not isinstance(m, torch.nn.Conv2d):
                raise ValueError(f"Conv2dSubsampling: module {i} of the Sequential is a {type(m).__name__}, not a "
                                 "Conv2d (optionally followed by a ReLU)")
            act = None
            if i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU):
                act, i = "relu", i + 1
            W, b, kw = Conv2d.pack_torch(m)
            if layers and kw["c_in"] != layers[-1]["c_out"]:
                raise ValueError(f"Conv2dSubsampling: module {i} takes {kw['c_in']} channels, the layer before it "
                                 f"makes {layers[-1]['c_out']}")
            if causal:
                kw["padding"] = ((kw["kernel"][0] - 1, 0), kw["padding"][1])
            kw.update(feat_in=F, act=act, weight=W, bias=b)
            F = conv2d_out_feats(Conv2d.make_desc(**{k: v for k, v in kw.items() if k not in ("weight", "bias")}))
            if F < 0:
                raise AsrError(-F, "asr_conv2d_out_feats")
            layers.append(kw)
            i += 1
        if not layers:
            raise ValueError("Conv2dSubsampling: no Conv2d in the Sequential")
        w, b = Conv2dSubsampling.pack_linear(out, layers[-1]["c_out"], F, scale)
        return layers, w, b

    @classmethod
    def from_torch(cls, conv, out, feat_in: int, scale: float = 1.0, causal: bool = False) -> "Conv2dSubsampling":
        """conv: a torch.nn.Sequential of Conv2d modules on [B][C][T][F], each
        optionally followed by a ReLU (fused into that layer); any other module
        is refused.  out: the torch.nn.Linear over the flattened (c, f) axis.
        causal: every layer's time padding becomes (kernel_t - 1, 0), the
        streamable form (a module that pads that way by hand before each
        unpadded-in-time convolution); the frequency padding stays."""
        layers, w, b = cls.pack_torch(conv, out, feat_in, scale, causal)
        return cls([Conv2d(**kw) for kw in layers], w, b)

    def frames(self, n: int) -> int:
        """Frames out for n frames in: the layers' out_frames chained."""
        for layer in self.layers:
            n = layer.out_frames(n)
        return n

    def forward(self, x, T: int, B: int, lengths=None, zero_padding: bool = True, stream: int = 0):
        """x time-major [T*B, >= feat_in * c_in] (a log-mel matrix as it stands
        for c_in = 1); lengths None, a sequence of B counts or a DeviceBytes of
        int32 [B].  Returns (out, T_out, out_lengths): a new DeviceMatrix
        [T_out*B, E], rows past each utterance's count zero when zero_padding
        (else the Linear's bias), and the DeviceBytes of int32 [B] that the
        encoder layers take as lengths (None when no lengths were given)."""
        if x.rows != T * B or x.cols < self.feat_in * self.c_in:
            raise ValueError(f"Conv2dSubsampling.forward: x is [{x.rows}, {x.cols}], expected [{T * B}, >= "
                             f"{self.feat_in * self.c_in}]")
        st = stream or 0
        lengths = _device_lengths_or_none(lengths)
        keep, h, t, ln = [lengths], x, T, lengths
        for i, layer in enumerate(self.layers):
            t_out = layer.out_frames(t)
            if t_out <= 0:
                raise AsrError(ASR_ERR_ARG if t_out == 0 else -t_out, "asr_conv2d_out_frames")
            o = self._scratch.get(f"h{i}", t_out * B, layer.feat_out * layer.desc.c_out)
            oln = None if ln is None else DeviceBytes(4 * B)
            conv2d_fwd(h, layer.W, layer.b, o, t, B, layer.desc, lengths=ln, out_lengths=oln, stream=st)
            keep.append(oln)
            h, t, ln = o, t_out, oln
        out = DeviceMatrix(t * B, self.E)
        linear_fwd(h, self.w_out, self.b_out, out, EPI_BIAS, st)
        if zero_padding and ln is not None:
            mask_rows(out, t, B, self.E, ln, st)
        self._keep = keep
        return out, t, ln


# ------------------------------------------------- attention and LayerNorm
ATTN_KEY_BLOCK = 64   # ASR_ATTN_KEY_BLOCK


class AttnDesc(ctypes.Structure):
    """asr_attn_desc (include/asr_amd.h)."""
    _fields_ = [("heads", _i), ("head_dim", _i), ("scale", _f), ("chunk", _i), ("left", _i), ("right", _i)]


def attn_desc(heads: int, head_dim: int, scale: float = 0.0, chunk: int = 1, left: int = -1,
              right: int = -1) -> AttnDesc:
    """An AttnDesc from keywords: scale 0 = 1/sqrt(head_dim); query p sees key r
    iff p//chunk - left <= r//chunk <= p//chunk + right (-1 drops that side)."""
    return AttnDesc(heads, head_dim, scale, chunk, left, right)


class ColumnView:
    """Columns [col, ...) of the rows of a device matrix, without owning them:
    ptr addresses (row 0, column col), cols stays the owner's row stride."""

    def __init__(self, m, col: int):
        assert 0 <= col < m.cols, (col, m.cols)
        self.ptr, self.rows, self.cols, self._keep = m.ptr + 4 * col, m.rows, m.cols, m
        self.col = col + int(getattr(m, "col", 0))


def _device_lengths_or_none(lengths):
    if lengths is None or isinstance(lengths, DeviceBytes):
        return lengths
    return device_lengths(lengths)


def attention_fwd(q, k, v, out, Tq: int, Tk: int, B: int, desc: AttnDesc, lengths: Optional[DeviceBytes] = None,
                  q_pos0: int = 0, k_pos0: int = 0, ldq: Optional[int] = None, ldk: Optional[int] = None,
                  ldv: Optional[int] = None, ldo: Optional[int] = None, stream: int = 0):
    """softmax(Q K^T scale) V per head over time (asr_attention_fwd): q, out
    [Tq*B, >= E] and k, v [Tk*B, >= E] time-major, E = heads*head_dim; anything
    with .ptr and .cols (the row stride unless ld* is given), so q, k and v may
    be ColumnViews of one [T*B, 3E] projection buffer; lengths from
    device_lengths(), in absolute frames."""
    ld = lambda m, given: int(m.cols if given is None else given)   # noqa: E731
    check(lib().asr_attention_fwd(ctypes.byref(desc), q.ptr, ld(q, ldq), k.ptr, ld(k, ldk), v.ptr, ld(v, ldv),
                                  lengths.ptr if lengths is not None else None, out.ptr, ld(out, ldo),
                                  Tq, q_pos0, Tk, k_pos0, B, stream), "asr_attention_fwd")
    return out


def rel_positional_encoding(max_left: int, max_right: int, E: int) -> np.ndarray:
    """The sinusoidal table of relative positions [max_left + max_right + 1, E]
    float32 in the order of ESPnet's / WeNet's / NeMo's pos_emb (flip(positive)
    followed by negative[1:]): row i is distance delta = max_left - i (query
    frame - key frame), from max_left down to -max_right, so distance 0 is row
    max_left.  The row of delta holds sin(delta w_k) at column 2k and
    cos(delta w_k) at column 2k + 1, w_k = 10000^(-2k / E); computed in float64
    on the host.  E even.  Host only: the relative-position attention that
    would read it is not built."""
    if max_left < 0 or max_right < 0 or E <= 0 or E % 2:
        raise ValueError(f"rel_positional_encoding: max_left {max_left}, max_right {max_right}, E {E}")
    delta = np.arange(max_left, -max_right - 1, -1, dtype=np.float64)[:, None]
    w = np.power(10000.0, -np.arange(0, E, 2, dtype=np.float64) / E)[None, :]
    out = np.empty((max_left + max_right + 1, E), np.float64)
    out[:, 0::2], out[:, 1::2] = np.sin(delta * w), np.cos(delta * w)
    return out.astype(np.float32)


def layernorm_fwd(x, out, T: int, B: int, N: int, gamma=None, beta=None, eps: float = 1e-5, res=None,
                  lengths: Optional[DeviceBytes] = None, stream: int = 0):
    """LayerNorm over the first N columns of each row of x (+ res) into out
    (asr_layernorm_fwd); x, res, out: anything with .ptr and .cols (the row
    stride); out may be x or res; rows past lengths become zeros."""
    opt = lambda m: m.ptr if m is not None else None   # noqa: E731
    check(lib().asr_layernorm_fwd(x.ptr, x.cols, opt(res), res.cols if res is not None else 0, opt(gamma),
                                  opt(beta), eps, opt(lengths), out.ptr, out.cols, T, B, N, stream),
          "asr_layernorm_fwd")
    return out


def mask_rows(x, T: int, B: int, N: int, lengths: Optional[DeviceBytes], stream: int = 0):
    """Zero the first N columns of rows t >= len[b] of x in place (asr_mask_rows)."""
    check(lib().asr_mask_rows(x.ptr, x.cols, lengths.ptr if lengths is not None else None, T, B, N, stream),
          "asr_mask_rows")
    return x


class _Scratch:
    """Device buffers of a layer, kept between calls and reallocated on a new shape."""

    def __init__(self):
        self._bufs = {}

    def get(self, name: str, rows: int, cols: int) -> DeviceMatrix:
        m = self._bufs.get(name)
        if m is None or (m.rows, m.cols) != (rows, cols):
            m = self._bufs[name] = DeviceMatrix(rows, cols)
        return m


class LayerNorm:
    """torch.nn.LayerNorm(N) over the columns of time-major rows for inference
    on asr_layernorm_fwd; weight / bias [N] or None (1 / 0)."""

    def __init__(self, N: int, eps: float = 1e-5, weight=None, bias=None):
        self.N, self.eps = int(N), float(eps)
        up = lambda a: None if a is None else DeviceMatrix.from_numpy(   # noqa: E731
            np.asarray(a, np.float32).reshape(self.N, 1))
        self.gamma, self.beta = up(weight), up(bias)
        self._keep = None

    @classmethod
    def from_torch(cls, ln) -> "LayerNorm":
        shape = tuple(ln.normalized_shape)
        if len(shape) != 1:
            raise ValueError(f"LayerNorm.from_torch: normalized_shape {shape} is not one dimension")
        host = lambda p: None if p is None else p.detach().cpu().float().numpy()   # noqa: E731
        return cls(shape[0], ln.eps, host(getattr(ln, "weight", None)), host(getattr(ln, "bias", None)))

    def forward(self, x, T: int, B: int, lengths=None, res=None, out=None, stream: int = 0):
        """LayerNorm(x + res) (res None: of x) of time-major x [T*B, N]; lengths
        None, a sequence of B counts or a DeviceBytes of int32 [B]: rows past
        them are zeros.  out defaults to a new DeviceMatrix; it may be x or res."""
        lengths = _device_lengths_or_none(lengths)
        out = DeviceMatrix(T * B, self.N) if out is None else out
        layernorm_fwd(x, out, T, B, self.N, self.gamma, self.beta, self.eps, res, lengths, stream or 0)
        self._keep = lengths
        return out


class MultiheadAttention:
    """torch.nn.MultiheadAttention(E, heads) as self-attention for inference:
    asr_linear_fwd to [T*B, 3E], one asr_attention_fwd on its three column
    ranges, asr_linear_fwd; time-major, no arithmetic here.  w_in [E, 3E] and
    w_out [E, E] in this library's [in][out] layout, b_in [3E], b_out [E]
    (zeros if None).  chunk / left / right: the window of asr_attn_desc
    (defaults: full attention).  Dropout is ignored."""

    def __init__(self, embed_dim: int, heads: int, w_in=None, b_in=None, w_out=None, b_out=None, chunk: int = 1,
                 left: int = -1, right: int = -1):
        E = int(embed_dim)
        if heads <= 0 or E <= 0 or E % heads:
            raise ValueError(f"MultiheadAttention: embed_dim {E} is not a multiple of heads {heads}")
        hd = E // heads
        if hd % 4 or hd > 128 or E > 4096:
            raise ValueError(f"MultiheadAttention: head_dim {hd} (% 4 == 0, <= 128) / embed_dim {E} (<= 4096) "
                             "outside what asr_attention_fwd takes")
        if chunk < 1 or left < -1 or right < -1:
            raise ValueError(f"MultiheadAttention: window chunk {chunk}, left {left}, right {right}")
        self.E, self.heads = E, heads
        self.desc = attn_desc(heads, hd, 0.0, chunk, left, right)
        self._xdesc = XAttnDesc(heads, hd, 0.0)      # the same heads and scale, for step()
        arr = lambda a, shape: (np.zeros(shape, np.float32) if a is None   # noqa: E731
                                else np.asarray(a, np.float32).reshape(shape))
        self.w_in, self.b_in = DeviceMatrix.from_numpy(arr(w_in, (E, 3 * E))), DeviceMatrix.from_numpy(
            arr(b_in, (3 * E, 1)))
        self.w_out, self.b_out = DeviceMatrix.from_numpy(arr(w_out, (E, E))), DeviceMatrix.from_numpy(
            arr(b_out, (E, 1)))
        self._scratch, self._keep = _Scratch(), None

    @staticmethod
    def pack_torch(mha):
        """(w_in [E, 3E], b_in [3E], w_out [E, E], b_out [E]) float32 from a
        torch.nn.MultiheadAttention: in_proj_weight [3E, E] and out_proj.weight
        [E, E] transposed into the [in][out] layout.  No device call."""
        E = mha.embed_dim
        if not getattr(mha, "_qkv_same_embed_dim", mha.kdim == E and mha.vdim == E):
            raise ValueError("MultiheadAttention.from_torch: kdim / vdim != embed_dim is not supported")
        if mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn:
            raise ValueError("MultiheadAttention.from_torch: bias_k / bias_v / add_zero_attn are not supported")
        host = lambda p: p.detach().cpu().float().numpy()   # noqa: E731
        w_in = np.ascontiguousarray(host(mha.in_proj_weight).T)
        b_in = host(mha.in_proj_bias) if mha.in_proj_bias is not None else np.zeros(3 * E, np.float32)
        w_out = np.ascontiguousarray(host(mha.out_proj.weight).T)
        b_out = host(mha.out_proj.bias) if mha.out_proj.bias is not None else np.zeros(E, np.float32)
        return w_in, b_in, w_out, b_out

    @classmethod
    def from_torch(cls, mha, chunk: int = 1, left: int = -1, right: int = -1) -> "MultiheadAttention":
        w_in, b_in, w_out, b_out = cls.pack_torch(mha)
        return cls(mha.embed_dim, mha.num_heads, w_in, b_in, w_out, b_out, chunk, left, right)

    def forward(self, x, T: int, B: int, lengths=None, out=None, zero_padding: bool = True, stream: int = 0):
        """Self-attention of time-major x [T*B, E]; lengths None, a sequence of B
        counts or a DeviceBytes of int32 [B].  Returns out [T*B, E] (a buffer of
        this layer, reused by its next call, unless given); rows past the lengths
        are zeros (asr_mask_rows after the output projection) unless
        zero_padding is False, in which case they hold the output bias."""
        E, M, st = self.E, T * B, stream or 0
        lengths = _device_lengths_or_none(lengths)
        qkv = self._scratch.get("qkv", M, 3 * E)
        ctx = self._scratch.get("ctx", M, E)
        out = self._scratch.get("out", M, E) if out is None else out
        linear_fwd(x, self.w_in, self.b_in, qkv, EPI_BIAS, st)
        attention_fwd(ColumnView(qkv, 0), ColumnView(qkv, E), ColumnView(qkv, 2 * E), ctx, T, T, B, self.desc,
                      lengths=lengths, stream=st)
        linear_fwd(ctx, self.w_out, self.b_out, out, EPI_BIAS, st)
        if zero_padding and lengths is not None:
            mask_rows(out, T, B, E, lengths, st)
        self._keep = lengths
        return out

    def step(self, x, N: int, cache, step: int, anc, out=None, stream: int = 0):
        """One autoregressive step of causal self-attention: x [N, E] is the
        row of step `step` of N hypotheses.  One fused QKV GEMM writes the row
        in place at rows step*N .. step*N + N - 1 of cache [max_len*N, 3E] (Q,
        K and V columns: no copy appends K / V), then asr_decode_attention_fwd
        over keys 0 .. step through the ancestry table anc (device int32
        [max_len][N], or a host table that is validated): entry [j][n] is the
        slot whose row j holds hypothesis n's key, so a beam reorder never
        moves the cache.  The layer must be causal over its whole history
        (chunk 1, left -1, right 0: ValueError otherwise).  Returns out [N, E]
        (a buffer of this layer unless given)."""
        E, N, step, st = self.E, int(N), int(step), stream or 0
        if (self.desc.chunk, self.desc.left, self.desc.right) != (1, -1, 0):
            raise ValueError("MultiheadAttention.step: the layer must be causal over its whole history (chunk 1, "
                             "left -1, right 0); a limited window is not built for the cache")
        _need_matrix("MultiheadAttention.step: x", x, N, E)
        if x.rows != N or x.cols != E:
            raise ValueError(f"MultiheadAttention.step: x is {x.rows} x {x.cols}, not N x E = {N} x {E}")
        if cache.cols != 3 * E or step < 0 or (step + 1) * N > cache.rows:
            raise ValueError(f"MultiheadAttention.step: cache is {cache.rows} x {cache.cols}; step {step} needs "
                             f"{(step + 1) * N} x {3 * E}")
        if _is_device(anc):
            _need_int32("MultiheadAttention.step: anc", anc, (step + 1) * N)
        else:                                # a host table is validated before the first device call
            anc = np.asarray(anc)[:step + 1]
            _host_table("MultiheadAttention.step: anc", anc, step + 1, N, 0, N)
        if out is not None:
            _need_matrix("MultiheadAttention.step: out", out, N, E)
        ctx = self._scratch.get("sctx", N, E)
        out = self._scratch.get("sout", N, E) if out is None else out
        row = RowView(cache, step * N, N)
        linear_fwd(x, self.w_in, self.b_in, row, EPI_BIAS, st)
        decode_attention_fwd(ColumnView(row, 0), ColumnView(cache, E), ColumnView(cache, 2 * E), ctx, N, step + 1, N,
                             self._xdesc, anc, ldc=N, stream=st)
        linear_fwd(ctx, self.w_out, self.b_out, out, EPI_BIAS, st)
        return out


class TransformerEncoderLayer:
    """torch.nn.TransformerEncoderLayer (ReLU feed-forward, norm_first either
    way) for inference, time-major: MultiheadAttention, two LayerNorms and two
    asr_linear_fwd (the first with bias + ReLU fused).  Post-norm uses the
    fused residual of asr_layernorm_fwd, pre-norm asr_matadd.  Dropout is
    ignored."""

    def __init__(self, attn: MultiheadAttention, norm1: LayerNorm, norm2: LayerNorm, w1, b1, w2, b2,
                 norm_first: bool = False):
        E = attn.E
        w1, w2 = np.asarray(w1, np.float32), np.asarray(w2, np.float32)
        F = w1.shape[1]
        assert w1.shape == (E, F) and w2.shape == (F, E), (w1.shape, w2.shape)
        self.E, self.F, self.norm_first = E, F, bool(norm_first)
        self.attn, self.norm1, self.norm2 = attn, norm1, norm2
        self.w1, self.w2 = DeviceMatrix.from_numpy(w1), DeviceMatrix.from_numpy(w2)
        self.b1 = DeviceMatrix.from_numpy(np.asarray(b1, np.float32).reshape(F, 1))
        self.b2 = DeviceMatrix.from_numpy(np.asarray(b2, np.float32).reshape(E, 1))
        self._scratch, self._keep = _Scratch(), None

    @staticmethod
    def pack_torch(layer):
        """(w1 [E, F], b1 [F], w2 [F, E], b2 [E]) float32 of the feed-forward
        of a torch.nn.TransformerEncoderLayer, in the [in][out] layout; raises
        ValueError for an activation other than ReLU.  No device call."""
        act = layer.activation
        name = getattr(act, "__name__", type(act).__name__).lower()
        if name != "relu":
            raise ValueError(f"TransformerEncoderLayer.from_torch: activation {name!r} is not supported (ReLU only)")
        host = lambda p: p.detach().cpu().float().numpy()   # noqa: E731
        bias = lambda lin: (host(lin.bias) if lin.bias is not None   # noqa: E731
                            else np.zeros(lin.out_features, np.float32))
        return (np.ascontiguousarray(host(layer.linear1.weight).T), bias(layer.linear1),
                np.ascontiguousarray(host(layer.linear2.weight).T), bias(layer.linear2))

    @classmethod
    def from_torch(cls, layer, chunk: int = 1, left: int = -1, right: int = -1) -> "TransformerEncoderLayer":
        w1, b1, w2, b2 = cls.pack_torch(layer)
        return cls(MultiheadAttention.from_torch(layer.self_attn, chunk, left, right),
                   LayerNorm.from_torch(layer.norm1), LayerNorm.from_torch(layer.norm2), w1, b1, w2, b2,
                   layer.norm_first)

    def forward(self, x, T: int, B: int, lengths=None, stream: int = 0) -> DeviceMatrix:
        """x time-major [T*B, E]; lengths None, a sequence of B counts or a
        DeviceBytes of int32 [B] (e.g. Conv1d.forward's out_lengths).  Returns a
        new DeviceMatrix [T*B, E] with zero rows past the lengths."""
        E, F, M, st = self.E, self.F, T * B, stream or 0
        lengths = _device_lengths_or_none(lengths)
        sc = self._scratch
        h, ff = sc.get("h", M, E), sc.get("ff", M, F)
        out = DeviceMatrix(M, E)
        if self.norm_first:
            n = sc.get("n", M, E)
            self.norm1.forward(x, T, B, lengths, out=n, stream=st)
            a = self.attn.forward(n, T, B, lengths, zero_padding=False, stream=st)
            check(lib().asr_matadd(x.ptr, a.ptr, h.ptr, M, E, 1.0, st), "asr_matadd")
            self.norm2.forward(h, T, B, lengths, out=n, stream=st)
            linear_fwd(n, self.w1, self.b1, ff, EPI_BIAS_RELU, st)
            linear_fwd(ff, self.w2, self.b2, n, EPI_BIAS, st)
            check(lib().asr_matadd(h.ptr, n.ptr, out.ptr, M, E, 1.0, st), "asr_matadd")
            if lengths is not None:
                mask_rows(out, T, B, E, lengths, st)
        else:
            a = self.attn.forward(x, T, B, lengths, zero_padding=False, stream=st)
            self.norm1.forward(a, T, B, lengths, res=x, out=h, stream=st)
            f2 = sc.get("f2", M, E)
            linear_fwd(h, self.w1, self.b1, ff, EPI_BIAS_RELU, st)
            linear_fwd(ff, self.w2, self.b2, f2, EPI_BIAS, st)
            self.norm2.forward(f2, T, B, lengths, res=h, out=out, stream=st)
        self._keep = lengths
        return out


# ------------------------------------- attention decoder (n-best rescoring)
class XAttnDesc(ctypes.Structure):
    """asr_xattn_desc (include/asr_amd.h)."""
    _fields_ = [("heads", _i), ("head_dim", _i), ("scale", _f)]


def xattn_desc(heads: int, head_dim: int, scale: float = 0.0) -> XAttnDesc:
    """An XAttnDesc: scale 0 = 1/sqrt(head_dim)."""
    return XAttnDesc(heads, head_dim, scale)


def _need_matrix(what: str, m, rows: int, cols: int, ld: Optional[int] = None) -> None:
    """ValueError unless the device matrix (or view) m holds the rows x cols
    floats a call will touch at row stride ld (default m.cols)."""
    stride = int(m.cols if ld is None else ld)
    col = int(getattr(m, "col", 0)) if ld is None else 0
    if rows < 1 or cols < 1 or stride < col + cols or (rows - 1) * stride + col + cols > int(m.rows) * int(m.cols):
        raise ValueError(f"{what}: needs {rows} rows x {cols} columns at row stride {stride}, got a buffer of "
                         f"{m.rows} x {m.cols}" + (f" from column {col}" if col else ""))


def _need_int32(what: str, d, n: int) -> None:
    if d is not None and d.nbytes < 4 * n:
        raise ValueError(f"{what}: needs {n} int32, got {d.nbytes} bytes")


def _device_int32_exact(what: str, a, n: int):
    """a device int32 [n] array from None, a DeviceBytes or a host sequence of exactly n values."""
    if a is None or isinstance(a, DeviceBytes):
        _need_int32(what, a, n)
        return a
    if len(a) != n:
        raise ValueError(f"{what}: {len(a)} values, not {n}")
    return device_lengths(a)


def cross_attention_fwd(q, k, v, out, U: int, N: int, T: int, B: int, desc: XAttnDesc, hyp_offsets, max_hyps: int,
                        q_lengths=None, k_lengths=None, ldq: Optional[int] = None, ldk: Optional[int] = None,
                        ldv: Optional[int] = None, ldo: Optional[int] = None, stream: int = 0):
    """Grouped cross-attention (asr_cross_attention_fwd): q, out [U*N, >= E]
    (row u*N + n: token u of hypothesis n), k, v [T*B, >= E] (row j*B + b:
    frame j of utterance b), E = heads*head_dim; anything with .ptr, .rows and
    .cols (the row stride unless ld* is given), so k and v may be ColumnViews
    of one [T*B, 2E] projection.  hyp_offsets: B + 1 values (a sequence or a
    DeviceBytes of int32), hypotheses off[b] .. off[b+1] - 1 belong to
    utterance b; max_hyps bounds their count per utterance.  q_lengths [N],
    k_lengths [B]: None, sequences or DeviceBytes.  Raises ValueError before
    any device call if a buffer is smaller than the rows and columns the call
    will touch."""
    U, N, T, B = int(U), int(N), int(T), int(B)
    E = int(desc.heads) * int(desc.head_dim)
    _need_matrix("cross_attention_fwd: q", q, U * N, E, ldq)
    _need_matrix("cross_attention_fwd: k", k, T * B, E, ldk)
    _need_matrix("cross_attention_fwd: v", v, T * B, E, ldv)
    _need_matrix("cross_attention_fwd: out", out, U * N, E, ldo)
    if hyp_offsets is None:
        raise ValueError("cross_attention_fwd: hyp_offsets is required")
    off = _device_int32_exact("cross_attention_fwd: hyp_offsets", hyp_offsets, B + 1)
    ql = _device_int32_exact("cross_attention_fwd: q_lengths", q_lengths, N)
    kl = _device_int32_exact("cross_attention_fwd: k_lengths", k_lengths, B)
    ld = lambda m, given: int(m.cols if given is None else given)   # noqa: E731
    opt = lambda d: d.ptr if d is not None else None   # noqa: E731
    check(lib().asr_cross_attention_fwd(ctypes.byref(desc), q.ptr, ld(q, ldq), k.ptr, ld(k, ldk), v.ptr, ld(v, ldv),
                                        opt(ql), opt(kl), off.ptr, int(max_hyps), out.ptr, ld(out, ldo), U, N, T, B,
                                        stream), "asr_cross_attention_fwd")
    out._xattn_keep = (off, ql, kl)      # host sequences were uploaded here: keep them until out goes
    return out


def token_score(logp, tokens, lengths, U: int, N: int, V: int, ld: Optional[int] = None,
                stream: int = 0) -> np.ndarray:
    """fp64 [N]: sum over u < lengths[n] of logp[u*N + n][tokens[u][n]]
    (asr_token_score), logp a device [U*N, >= V] log-softmax buffer that stays
    on the device; tokens int [U][N] on the host; lengths [N] or None (= U).
    A token outside [0, V) gives -inf.  Only the N doubles are copied back."""
    U, N, V = int(U), int(N), int(V)
    _need_matrix("token_score: logp", logp, U * N, V, ld)
    tok = np.ascontiguousarray(tokens, dtype=np.int32)
    if tok.size != U * N:
        raise ValueError(f"token_score: {tok.size} tokens, not U*N = {U * N}")
    if lengths is not None and len(lengths) != N:
        raise ValueError(f"token_score: {len(lengths)} lengths, not N = {N}")
    d_tok = _upload(tok, stream)
    d_len = None if lengths is None else _upload(np.ascontiguousarray(lengths, dtype=np.int32), stream)
    d_out = DeviceBytes(8 * N)
    check(lib().asr_token_score(logp.ptr, int(logp.cols if ld is None else ld), d_tok.ptr,
                                d_len.ptr if d_len is not None else None, d_out.ptr, U, N, V, stream),
          "asr_token_score")
    return _download(d_out, N, np.float64, stream)


# ----------------------------------- attention decoder (autoregressive step)
ATTN_BEAM_MAX_K = 16   # ASR_ATTN_BEAM_MAX_K


class AttnBeamDesc(ctypes.Structure):
    """asr_attn_beam_desc (include/asr_amd.h)."""
    _fields_ = [("B", _i), ("K", _i), ("V", _i), ("max_len", _i), ("step", _i), ("eos", _i)]


def attn_beam_desc(B: int, K: int, V: int, max_len: int, step: int, eos: int) -> AttnBeamDesc:
    return AttnBeamDesc(B, K, V, max_len, step, eos)


class RowView:
    """Rows [row0, row0 + rows) of a device matrix, without owning them."""

    def __init__(self, m, row0: int, rows: int):
        if row0 < 0 or rows < 1 or row0 + rows > m.rows:
            raise ValueError(f"RowView: rows [{row0}, {row0 + rows}) of a buffer of {m.rows}")
        self.ptr, self.rows, self.cols, self._keep = m.ptr + 4 * row0 * m.cols, int(rows), m.cols, m
        self.nbytes = 4 * self.rows * self.cols


class Int32View:
    """n int32 of a device buffer from element first on, without owning them."""

    def __init__(self, d, first: int, n: int):
        if first < 0 or n < 0 or 4 * (first + n) > d.nbytes:
            raise ValueError(f"Int32View: elements [{first}, {first + n}) of a buffer of {d.nbytes} bytes")
        self.ptr, self.nbytes, self._keep = d.ptr + 4 * first, 4 * n, d


def _is_device(a) -> bool:
    return hasattr(a, "ptr") and hasattr(a, "nbytes")


def _host_table(what: str, a, rows: int, cols: int, lo: int, hi: int):
    """None for a device buffer (its size checked); a host table validated
    (shape, every value in [lo, hi)) as a contiguous int32 array to upload."""
    if _is_device(a):
        _need_int32(what, a, rows * cols)
        return None
    t = np.asarray(a)
    if t.shape != (rows, cols) and not (rows == 1 and t.shape == (cols,)):
        raise ValueError(f"{what}: shape {t.shape}, not ({rows}, {cols})")
    if t.size and (t.min() < lo or t.max() >= hi):
        raise ValueError(f"{what}: a value outside [{lo}, {hi})")
    return np.ascontiguousarray(t, dtype=np.int32)


def decode_attention_fwd(q, k, v, out, N: int, Tk: int, S: int, desc: XAttnDesc, cols, ldc: int = 0, lengths=None,
                         ldq: Optional[int] = None, ldk: Optional[int] = None, ldv: Optional[int] = None,
                         ldo: Optional[int] = None, stream: int = 0):
    """One query per hypothesis over a K/V cache (asr_decode_attention_fwd):
    q, out [N, >= E], k, v [Tk*S, >= E] (key j of column c: row j*S + c); E =
    heads*head_dim; anything with .ptr, .rows and .cols (the row stride unless
    ld* is given).  cols: with ldc = 0 the column of each hypothesis, [N]; with
    ldc >= N the [Tk][ldc] table whose entry [j][n] is the column of hypothesis
    n's key j.  A host table is validated (every value in [0, S)) and uploaded;
    a device buffer (DeviceBytes, Int32View) is used as it is and clamped by
    the kernel.  lengths [N]: None (= Tk), a host sequence or a device buffer.
    Raises ValueError before any device call if a buffer is smaller than what
    the call will touch."""
    N, Tk, S, ldc = int(N), int(Tk), int(S), int(ldc)
    E = int(desc.heads) * int(desc.head_dim)
    if N < 1 or Tk < 1 or S < 1:
        raise ValueError(f"decode_attention_fwd: N {N}, Tk {Tk}, S {S}")
    if ldc != 0 and ldc < N:
        raise ValueError(f"decode_attention_fwd: ldc {ldc} is neither 0 nor >= N = {N}")
    _need_matrix("decode_attention_fwd: q", q, N, E, ldq)
    _need_matrix("decode_attention_fwd: k", k, Tk * S, E, ldk)
    _need_matrix("decode_attention_fwd: v", v, Tk * S, E, ldv)
    _need_matrix("decode_attention_fwd: out", out, N, E, ldo)
    if cols is None:
        raise ValueError("decode_attention_fwd: cols is required")
    if ldc != 0 and _is_device(cols):
        _need_int32("decode_attention_fwd: cols", cols, (Tk - 1) * ldc + N)
        host_cols = None
    else:
        host_cols = _host_table("decode_attention_fwd: cols", cols, Tk if ldc else 1, ldc if ldc else N, 0, S)
    if lengths is not None and not _is_device(lengths) and len(lengths) != N:
        raise ValueError(f"decode_attention_fwd: {len(lengths)} lengths, not N = {N}")
    _need_int32("decode_attention_fwd: lengths", lengths if _is_device(lengths) else None, N)
    d_cols = cols if host_cols is None else _upload(host_cols, stream)
    ln = lengths if lengths is None or _is_device(lengths) else device_lengths(lengths)
    ld = lambda m, given: int(m.cols if given is None else given)   # noqa: E731
    check(lib().asr_decode_attention_fwd(ctypes.byref(desc), q.ptr, ld(q, ldq), k.ptr, ld(k, ldk), v.ptr, ld(v, ldv),
                                         d_cols.ptr, ldc, ln.ptr if ln is not None else None, out.ptr, ld(out, ldo),
                                         N, Tk, S, stream), "asr_decode_attention_fwd")
    out._dattn_keep = (d_cols, ln)       # host tables were uploaded here: keep them until out goes
    return out


def embed_fwd(emb, pe, tokens, pos, out, R: int, E: int, V: int, P: int = 0, scale: float = 1.0,
              ldo: Optional[int] = None, stream: int = 0):
    """out[r] = fp32(float64(emb[tokens[r]]) * scale + pe[pos[r]]) on the
    device (asr_embed_fwd): emb a device fp32 [V, E] matrix, pe a device fp64
    [P, E] buffer (DeviceBytes) or None (0), tokens / pos device int32 [R] or
    host sequences (uploaded as they are: a token outside [0, V) or a position
    outside [0, P) gives a zero row), out [R, >= E]."""
    R, E, V, P = int(R), int(E), int(V), int(P)
    if R < 1 or E < 1 or V < 1:
        raise ValueError(f"embed_fwd: R {R}, E {E}, V {V}")
    _need_matrix("embed_fwd: emb", emb, V, E)
    _need_matrix("embed_fwd: out", out, R, E, ldo)
    if pe is not None and (P < 1 or pe.nbytes < 8 * P * E):
        raise ValueError(f"embed_fwd: pe needs {P} x {E} float64, got {pe.nbytes} bytes")
    if pe is not None and pos is None:
        raise ValueError("embed_fwd: pe needs pos")
    if tokens is None:
        raise ValueError("embed_fwd: tokens is required")
    for what, a in (("tokens", tokens), ("pos", pos)):
        if _is_device(a):
            _need_int32(f"embed_fwd: {what}", a, R)
        elif a is not None and len(a) != R:
            raise ValueError(f"embed_fwd: {len(a)} {what}, not R = {R}")
    up = lambda a: a if a is None or _is_device(a) else device_lengths(a)   # noqa: E731
    tk, ps = up(tokens), up(pos)
    check(lib().asr_embed_fwd(emb.ptr, emb.cols, pe.ptr if pe is not None else None, E, tk.ptr,
                              ps.ptr if ps is not None else None, float(scale), out.ptr,
                              int(out.cols if ldo is None else ldo), R, E, V, P, stream), "asr_embed_fwd")
    out._embed_keep = (tk, ps)
    return out


def attn_beam_step(desc: AttnBeamDesc, logp, scores, finished, tokens_in, anc_in, scores_out, finished_out, parent,
                   token, tokens_out, anc_out, all_finished, ld: Optional[int] = None, stream: int = 0) -> None:
    """One prune of the attention beam search on the device
    (asr_attn_beam_step): every argument a device buffer (logp a matrix [N, >=
    V], the rest anything with .ptr and .nbytes), sizes checked here."""
    N, rows = desc.B * desc.K, desc.max_len * desc.B * desc.K
    if N < 1 or rows < 1:
        raise ValueError(f"attn_beam_step: B {desc.B}, K {desc.K}, max_len {desc.max_len}")
    _need_matrix("attn_beam_step: logp", logp, N, max(int(desc.V), 1), ld)
    for what, d, n, width in (("scores", scores, N, 8), ("finished", finished, N, 4), ("tokens_in", tokens_in, rows, 4),
                              ("anc_in", anc_in, rows, 4), ("scores_out", scores_out, N, 8),
                              ("finished_out", finished_out, N, 4), ("parent", parent, N, 4), ("token", token, N, 4),
                              ("tokens_out", tokens_out, rows, 4), ("anc_out", anc_out, rows, 4),
                              ("all_finished", all_finished, 1, 4)):
        if d is None or d.nbytes < width * n:
            raise ValueError(f"attn_beam_step: {what} needs {width * n} bytes")
    check(lib().asr_attn_beam_step(ctypes.byref(desc), logp.ptr, int(logp.cols if ld is None else ld), scores.ptr,
                                   finished.ptr, tokens_in.ptr, anc_in.ptr, scores_out.ptr, finished_out.ptr,
                                   parent.ptr, token.ptr, tokens_out.ptr, anc_out.ptr, all_finished.ptr, stream),
          "asr_attn_beam_step")


def attn_beam_step_host(desc: AttnBeamDesc, logp, scores, finished, tokens_in, anc_in):
    """The same prune on the host (asr_attn_beam_step_host), the CPU path:
    logp float32 [N, V], scores float64 [N], finished int [N], tokens_in /
    anc_in int [max_len][N].  Returns (scores, finished, parent, token,
    tokens_out, anc_out, live): the out tables start as copies of the in tables
    (rows past step + 1 keep them), live = the live unfinished slots."""
    N, L = desc.B * desc.K, desc.max_len
    logp = np.ascontiguousarray(logp, dtype=np.float32)
    if logp.ndim != 2 or logp.shape[0] != N or logp.shape[1] < max(desc.V, 1):
        raise ValueError(f"attn_beam_step_host: logp {logp.shape}, not [{N}, >= {desc.V}]")
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    finished = np.ascontiguousarray(finished, dtype=np.int32)
    tokens_in = np.ascontiguousarray(tokens_in, dtype=np.int32)
    anc_in = np.ascontiguousarray(anc_in, dtype=np.int32)
    if scores.shape != (N,) or finished.shape != (N,):
        raise ValueError(f"attn_beam_step_host: scores {scores.shape} / finished {finished.shape}, not ({N},)")
    if tokens_in.shape != (L, N) or anc_in.shape != (L, N):
        raise ValueError(f"attn_beam_step_host: tables {tokens_in.shape} / {anc_in.shape}, not ({L}, {N})")
    so, fo = np.empty(N, np.float64), np.empty(N, np.int32)
    par, tok = np.empty(N, np.int32), np.empty(N, np.int32)
    tout, aout, live = tokens_in.copy(), anc_in.copy(), np.zeros(1, np.int32)
    check(lib().asr_attn_beam_step_host(ctypes.byref(desc), _ptr(logp), logp.shape[1], _ptr(scores), _ptr(finished),
                                        _ptr(tokens_in), _ptr(anc_in), _ptr(so), _ptr(fo), _ptr(par), _ptr(tok),
                                        _ptr(tout), _ptr(aout), _ptr(live)), "asr_attn_beam_step_host")
    return so, fo, par, tok, tout, aout, int(live[0])


class CrossAttention:
    """torch.nn.MultiheadAttention(E, heads) as the encoder-decoder attention
    of a rescoring decoder: N hypotheses (the queries' batch) attend to the
    memories of B utterances through asr_cross_attention_fwd, so the memory's
    K / V projection runs once per utterance (project_memory) and not once per
    hypothesis.  w_q [E, E], w_kv [E, 2E] (K columns first) and w_out [E, E] in
    this library's [in][out] layout, b_q [E], b_kv [2E], b_out [E] (zeros if
    None).  No arithmetic here; dropout is ignored."""

    def __init__(self, embed_dim: int, heads: int, w_q=None, b_q=None, w_kv=None, b_kv=None, w_out=None,
                 b_out=None):
        E = int(embed_dim)
        if heads <= 0 or E <= 0 or E % heads:
            raise ValueError(f"CrossAttention: embed_dim {E} is not a multiple of heads {heads}")
        hd = E // heads
        if hd % 4 or hd > 128 or E > 4096:
            raise ValueError(f"CrossAttention: head_dim {hd} (% 4 == 0, <= 128) / embed_dim {E} (<= 4096) "
                             "outside what asr_cross_attention_fwd takes")
        self.E, self.heads = E, heads
        self.desc = xattn_desc(heads, hd, 0.0)
        arr = lambda a, shape: (np.zeros(shape, np.float32) if a is None   # noqa: E731
                                else np.asarray(a, np.float32).reshape(shape))
        up = lambda a, shape: DeviceMatrix.from_numpy(arr(a, shape))   # noqa: E731
        self.w_q, self.b_q = up(w_q, (E, E)), up(b_q, (E, 1))
        self.w_kv, self.b_kv = up(w_kv, (E, 2 * E)), up(b_kv, (2 * E, 1))
        self.w_out, self.b_out = up(w_out, (E, E)), up(b_out, (E, 1))
        self._scratch, self._keep = _Scratch(), None

    @staticmethod
    def pack_torch(mha):
        """(w_q [E, E], b_q [E], w_kv [E, 2E], b_kv [2E], w_out [E, E], b_out
        [E]) float32 from a torch.nn.MultiheadAttention: MultiheadAttention.
        pack_torch's arrays (and its refusals) with in_proj split into the
        query's columns and the memory's.  No device call."""
        w_in, b_in, w_out, b_out = MultiheadAttention.pack_torch(mha)
        E = mha.embed_dim
        return (np.ascontiguousarray(w_in[:, :E]), np.ascontiguousarray(b_in[:E]),
                np.ascontiguousarray(w_in[:, E:]), np.ascontiguousarray(b_in[E:]), w_out, b_out)

    @staticmethod
    def pack_linears(linear_q, linear_k, linear_v, linear_out):
        """The same six arrays from the four torch.nn.Linear modules of a
        toolkit attention (ESPnet's / WeNet's MultiHeadedAttention: linear_q,
        linear_k, linear_v, linear_out).  No device call."""
        (wq, bq), (wk, bk), (wv, bv), (wo, bo) = (_torch_linear(m) for m in (linear_q, linear_k, linear_v,
                                                                             linear_out))
        E = wq.shape[0]
        if any(w.shape != (E, E) for w in (wq, wk, wv, wo)):
            raise ValueError("CrossAttention.pack_linears: the four linears are not all E -> E")
        return (wq, bq, np.ascontiguousarray(np.concatenate([wk, wv], axis=1)), np.concatenate([bk, bv]), wo, bo)

    @classmethod
    def from_torch(cls, mha) -> "CrossAttention":
        return cls(mha.embed_dim, mha.num_heads, *cls.pack_torch(mha))

    def project_memory(self, memory, T: int, B: int, out=None, stream: int = 0):
        """K and V of the encoder output memory [T*B, E] (row j*B + b: frame j
        of utterance b) as one [T*B, 2E] buffer, computed once per batch of
        utterances and passed to forward() as kv."""
        E, M = self.E, int(T) * int(B)
        _need_matrix("CrossAttention.project_memory: memory", memory, M, E)
        if memory.rows != M or memory.cols != E:
            raise ValueError(f"CrossAttention.project_memory: memory is {memory.rows} x {memory.cols}, not "
                             f"T*B x E = {M} x {E}")
        out = DeviceMatrix(M, 2 * E) if out is None else out
        _need_matrix("CrossAttention.project_memory: out", out, M, 2 * E)
        return linear_fwd(memory, self.w_kv, self.b_kv, out, EPI_BIAS, stream or 0)

    def forward(self, x, U: int, N: int, kv, T: int, B: int, q_lengths=None, k_lengths=None, hyp_offsets=None,
                max_hyps: Optional[int] = None, out=None, zero_padding: bool = True, stream: int = 0):
        """Attention of the hypotheses' x [U*N, E] (row u*N + n) over kv =
        project_memory(...) [T*B, 2E]; q_lengths [N], k_lengths [B] and
        hyp_offsets [B + 1] as cross_attention_fwd's; max_hyps defaults to N.
        Returns out [U*N, E] (a buffer of this layer, reused by its next call,
        unless given); rows past q_lengths are zeros unless zero_padding is
        False, in which case they hold the output bias."""
        E, M, st = self.E, int(U) * int(N), stream or 0
        _need_matrix("CrossAttention.forward: x", x, M, E)
        if x.rows != M or x.cols != E:
            raise ValueError(f"CrossAttention.forward: x is {x.rows} x {x.cols}, not U*N x E = {M} x {E}")
        _need_matrix("CrossAttention.forward: kv", kv, int(T) * int(B), 2 * E)
        if kv.cols != 2 * E:
            raise ValueError(f"CrossAttention.forward: kv has {kv.cols} columns, not 2E = {2 * E}")
        q_lengths = _device_int32_exact("CrossAttention.forward: q_lengths", q_lengths, N)
        k_lengths = _device_int32_exact("CrossAttention.forward: k_lengths", k_lengths, B)
        hyp_offsets = _device_int32_exact("CrossAttention.forward: hyp_offsets", hyp_offsets, B + 1)
        qp, ctx = self._scratch.get("q", M, E), self._scratch.get("ctx", M, E)
        out = self._scratch.get("out", M, E) if out is None else out
        _need_matrix("CrossAttention.forward: out", out, M, E)
        linear_fwd(x, self.w_q, self.b_q, qp, EPI_BIAS, st)
        cross_attention_fwd(qp, ColumnView(kv, 0), ColumnView(kv, E), ctx, U, N, T, B, self.desc, hyp_offsets,
                            N if max_hyps is None else max_hyps, q_lengths, k_lengths, stream=st)
        linear_fwd(ctx, self.w_out, self.b_out, out, EPI_BIAS, st)
        if zero_padding and q_lengths is not None:
            mask_rows(out, U, N, E, q_lengths, st)
        self._keep = (q_lengths, k_lengths, hyp_offsets)
        return out

    def step(self, x, N: int, kv, T: int, B: int, hyp_offsets, max_hyps: Optional[int] = None, k_lengths=None,
             out=None, stream: int = 0):
        """One autoregressive step: the single rows x [N, E] of N hypotheses
        (ordered by utterance) attend to kv = project_memory(...) [T*B, 2E],
        computed once per search; hyp_offsets [B + 1] and k_lengths [B] as
        forward()'s.  This is forward() at U = 1 without q_lengths and without
        the row mask: asr_cross_attention_fwd, which stages an utterance's K /
        V once for all of its hypotheses, measured 2.4 to 5 times faster here
        than asr_decode_attention_fwd with ldc = 0, which re-reads them per
        hypothesis.  Returns out [N, E] (a buffer of
        this layer unless given); a hypothesis of an utterance with no frames
        gets the output bias."""
        E, N, st = self.E, int(N), stream or 0
        _need_matrix("CrossAttention.step: x", x, N, E)
        if x.rows != N or x.cols != E:
            raise ValueError(f"CrossAttention.step: x is {x.rows} x {x.cols}, not N x E = {N} x {E}")
        _need_matrix("CrossAttention.step: kv", kv, int(T) * int(B), 2 * E)
        if kv.cols != 2 * E:
            raise ValueError(f"CrossAttention.step: kv has {kv.cols} columns, not 2E = {2 * E}")
        if out is not None:
            _need_matrix("CrossAttention.step: out", out, N, E)
        if hyp_offsets is None:
            raise ValueError("CrossAttention.step: hyp_offsets is required")
        for what, a, n in (("hyp_offsets", hyp_offsets, int(B) + 1), ("k_lengths", k_lengths, int(B))):
            if _is_device(a):
                _need_int32(f"CrossAttention.step: {what}", a, n)
            elif a is not None and len(a) != n:
                raise ValueError(f"CrossAttention.step: {len(a)} {what}, not {n}")
        off = hyp_offsets if _is_device(hyp_offsets) else device_lengths(hyp_offsets)
        kl = k_lengths if k_lengths is None or _is_device(k_lengths) else device_lengths(k_lengths)
        qp, ctx = self._scratch.get("sq", N, E), self._scratch.get("sctx", N, E)
        out = self._scratch.get("sout", N, E) if out is None else out
        linear_fwd(x, self.w_q, self.b_q, qp, EPI_BIAS, st)
        cross_attention_fwd(qp, ColumnView(kv, 0), ColumnView(kv, E), ctx, 1, N, T, B, self.desc, off,
                            N if max_hyps is None else max_hyps, None, kl, stream=st)
        linear_fwd(ctx, self.w_out, self.b_out, out, EPI_BIAS, st)
        self._keep = (off, kl)
        return out


class TransformerDecoderLayer:
    """torch.nn.TransformerDecoderLayer (ReLU feed-forward, norm_first either
    way) for teacher-forced scoring, time-major with the hypotheses as the
    batch: causal MultiheadAttention over the tokens -> CrossAttention over
    the utterance's memory -> feed-forward, three LayerNorms; it mirrors
    TransformerEncoderLayer (post-norm uses the fused residual of
    asr_layernorm_fwd, pre-norm asr_matadd).  The plain constructor takes the
    packed parts, so an ESPnet / WeNet DecoderLayer (normalize_before =
    norm_first, concat_after False) loads through from_linears.  GELU is not
    built; dropout is ignored."""

    def __init__(self, self_attn: MultiheadAttention, cross_attn: CrossAttention, norm1: LayerNorm,
                 norm2: LayerNorm, norm3: LayerNorm, w1, b1, w2, b2, norm_first: bool = False):
        E = self_attn.E
        w1, w2 = np.asarray(w1, np.float32), np.asarray(w2, np.float32)
        F = w1.shape[1]
        if cross_attn.E != E or any(n.N != E for n in (norm1, norm2, norm3)):
            raise ValueError("TransformerDecoderLayer: the attentions and norms are not all over the same E")
        if w1.shape != (E, F) or w2.shape != (F, E):
            raise ValueError(f"TransformerDecoderLayer: feed-forward shapes {w1.shape}, {w2.shape}")
        d = self_attn.desc
        if (d.chunk, d.left, d.right) != (1, -1, 0):
            raise ValueError("TransformerDecoderLayer: self_attn must be causal (chunk 1, left -1, right 0)")
        self.E, self.F, self.norm_first = E, F, bool(norm_first)
        self.self_attn, self.cross_attn = self_attn, cross_attn
        self.norm1, self.norm2, self.norm3 = norm1, norm2, norm3
        self.w1, self.w2 = DeviceMatrix.from_numpy(w1), DeviceMatrix.from_numpy(w2)
        self.b1 = DeviceMatrix.from_numpy(np.asarray(b1, np.float32).reshape(F, 1))
        self.b2 = DeviceMatrix.from_numpy(np.asarray(b2, np.float32).reshape(E, 1))
        self._scratch, self._keep = _Scratch(), None

    @classmethod
    def from_torch(cls, layer) -> "TransformerDecoderLayer":
        """From a torch.nn.TransformerDecoderLayer; ReLU only (ValueError
        otherwise), norm_first either way, the refusals of
        MultiheadAttention.pack_torch for both attentions."""
        w1, b1, w2, b2 = TransformerEncoderLayer.pack_torch(layer)
        return cls(MultiheadAttention.from_torch(layer.self_attn, 1, -1, 0),
                   CrossAttention.from_torch(layer.multihead_attn), LayerNorm.from_torch(layer.norm1),
                   LayerNorm.from_torch(layer.norm2), LayerNorm.from_torch(layer.norm3), w1, b1, w2, b2,
                   layer.norm_first)

    @classmethod
    def from_linears(cls, heads: int, self_attn, src_attn, norm1, norm2, norm3, w_1, w_2,
                     normalize_before: bool = True) -> "TransformerDecoderLayer":
        """From the parts of a toolkit DecoderLayer (ESPnet / WeNet): self_attn
        and src_attn each (linear_q, linear_k, linear_v, linear_out) torch
        Linears, three LayerNorms, the feed-forward's two Linears (ReLU between
        them).  That layout follows the toolkits' published forward; it is
        tested on a stand-in module (tests/attention_decoder_reference.py),
        never on the toolkits themselves."""
        wq, bq, wkv, bkv, wo, bo = CrossAttention.pack_linears(*self_attn)
        E = wq.shape[0]
        sa = MultiheadAttention(E, heads, np.concatenate([wq, wkv], axis=1), np.concatenate([bq, bkv]), wo, bo,
                                1, -1, 0)
        ca = CrossAttention(E, heads, *CrossAttention.pack_linears(*src_attn))
        (w1, b1), (w2, b2) = _torch_linear(w_1), _torch_linear(w_2)
        return cls(sa, ca, LayerNorm.from_torch(norm1), LayerNorm.from_torch(norm2), LayerNorm.from_torch(norm3),
                   w1, b1, w2, b2, normalize_before)

    def forward(self, x, U: int, N: int, kv, T: int, B: int, q_lengths=None, k_lengths=None, hyp_offsets=None,
                max_hyps: Optional[int] = None, out=None, stream: int = 0) -> DeviceMatrix:
        """x [U*N, E] (row u*N + n: token u of hypothesis n), kv =
        cross_attn.project_memory(memory, T, B); q_lengths [N], k_lengths [B],
        hyp_offsets [B + 1] as cross_attention_fwd's.  Returns out (a new
        DeviceMatrix [U*N, E] unless given; not x) with zero rows past
        q_lengths."""
        E, F, M, st = self.E, self.F, int(U) * int(N), stream or 0
        _need_matrix("TransformerDecoderLayer.forward: x", x, M, E)
        if x.rows != M or x.cols != E:
            raise ValueError(f"TransformerDecoderLayer.forward: x is {x.rows} x {x.cols}, not U*N x E = {M} x {E}")
        _need_matrix("TransformerDecoderLayer.forward: kv", kv, int(T) * int(B), 2 * E)
        ql = _device_int32_exact("TransformerDecoderLayer.forward: q_lengths", q_lengths, N)
        kl = _device_int32_exact("TransformerDecoderLayer.forward: k_lengths", k_lengths, B)
        off = _device_int32_exact("TransformerDecoderLayer.forward: hyp_offsets", hyp_offsets, B + 1)
        sc = self._scratch
        h, h2, ff = sc.get("h", M, E), sc.get("h2", M, E), sc.get("ff", M, F)
        add = lambda a, b, z: check(lib().asr_matadd(a.ptr, b.ptr, z.ptr, M, E, 1.0, st), "asr_matadd")   # noqa: E731
        cross = lambda q: self.cross_attn.forward(q, U, N, kv, T, B, ql, kl, off, max_hyps,   # noqa: E731
                                                  zero_padding=False, stream=st)
        out = DeviceMatrix(M, E) if out is None else out
        _need_matrix("TransformerDecoderLayer.forward: out", out, M, E)
        if out is x:
            raise ValueError("TransformerDecoderLayer.forward: out must not be x")
        if self.norm_first:
            n = sc.get("n", M, E)
            self.norm1.forward(x, U, N, ql, out=n, stream=st)
            add(x, self.self_attn.forward(n, U, N, ql, zero_padding=False, stream=st), h)
            self.norm2.forward(h, U, N, ql, out=n, stream=st)
            add(h, cross(n), h2)
            self.norm3.forward(h2, U, N, ql, out=n, stream=st)
            linear_fwd(n, self.w1, self.b1, ff, EPI_BIAS_RELU, st)
            linear_fwd(ff, self.w2, self.b2, n, EPI_BIAS, st)
            add(h2, n, out)
            if ql is not None:
                mask_rows(out, U, N, E, ql, st)
        else:
            a = self.self_attn.forward(x, U, N, ql, zero_padding=False, stream=st)
            self.norm1.forward(a, U, N, ql, res=x, out=h, stream=st)
            self.norm2.forward(cross(h), U, N, ql, res=h, out=h2, stream=st)
            f2 = sc.get("f2", M, E)
            linear_fwd(h2, self.w1, self.b1, ff, EPI_BIAS_RELU, st)
            linear_fwd(ff, self.w2, self.b2, f2, EPI_BIAS, st)
            self.norm3.forward(f2, U, N, ql, res=h2, out=out, stream=st)
        self._keep = (ql, kl, off)
        return out

    def step(self, x, N: int, cache, step: int, anc, kv, T: int, B: int, hyp_offsets, max_hyps: Optional[int] = None,
             k_lengths=None, out=None, stream: int = 0) -> DeviceMatrix:
        """forward() for the single row of step `step` of N hypotheses, on the
        K/V cache: MultiheadAttention.step over cache [max_len*N, 3E] through
        the ancestry table anc, CrossAttention.step over kv with hyp_offsets
        [B + 1] and the utterances' frames k_lengths [B], the feed-forward.
        Returns out (a new DeviceMatrix [N, E] unless given; not x)."""
        E, F, M, st = self.E, self.F, int(N), stream or 0
        _need_matrix("TransformerDecoderLayer.step: x", x, M, E)
        if x.rows != M or x.cols != E:
            raise ValueError(f"TransformerDecoderLayer.step: x is {x.rows} x {x.cols}, not N x E = {M} x {E}")
        _need_matrix("TransformerDecoderLayer.step: kv", kv, int(T) * int(B), 2 * E)
        if cache.cols != 3 * E or step < 0 or (int(step) + 1) * M > cache.rows:
            raise ValueError(f"TransformerDecoderLayer.step: cache is {cache.rows} x {cache.cols}; step {step} needs "
                             f"{(int(step) + 1) * M} x {3 * E}")
        if out is not None:
            _need_matrix("TransformerDecoderLayer.step: out", out, M, E)
        if out is x:
            raise ValueError("TransformerDecoderLayer.step: out must not be x")
        sc = self._scratch
        h, h2, ff = sc.get("sh", M, E), sc.get("sh2", M, E), sc.get("sff", M, F)
        add = lambda a, b, z: check(lib().asr_matadd(a.ptr, b.ptr, z.ptr, M, E, 1.0, st), "asr_matadd")   # noqa: E731
        own = lambda q: self.self_attn.step(q, M, cache, step, anc, stream=st)   # noqa: E731
        cross = lambda q: self.cross_attn.step(q, M, kv, T, B, hyp_offsets, max_hyps, k_lengths,   # noqa: E731
                                               stream=st)
        out = DeviceMatrix(M, E) if out is None else out
        if self.norm_first:
            n = sc.get("sn", M, E)
            self.norm1.forward(x, 1, M, None, out=n, stream=st)
            add(x, own(n), h)
            self.norm2.forward(h, 1, M, None, out=n, stream=st)
            add(h, cross(n), h2)
            self.norm3.forward(h2, 1, M, None, out=n, stream=st)
            linear_fwd(n, self.w1, self.b1, ff, EPI_BIAS_RELU, st)
            linear_fwd(ff, self.w2, self.b2, n, EPI_BIAS, st)
            add(h2, n, out)
        else:
            self.norm1.forward(own(x), 1, M, None, res=x, out=h, stream=st)
            self.norm2.forward(cross(h), 1, M, None, res=h, out=h2, stream=st)
            f2 = sc.get("sf2", M, E)
            linear_fwd(h2, self.w1, self.b1, ff, EPI_BIAS_RELU, st)
            linear_fwd(ff, self.w2, self.b2, f2, EPI_BIAS, st)
            self.norm3.forward(f2, 1, M, None, res=h2, out=out, stream=st)
        return out


def sinusoidal_positional_encoding(length: int, E: int) -> np.ndarray:
    """The toolkits' absolute PositionalEncoding table [length, E] float64:
    sin(pos w_k) at column 2k, cos(pos w_k) at column 2k + 1, w_k =
    10000^(-2k / E).  E even."""
    if length < 0 or E <= 0 or E % 2:
        raise ValueError(f"sinusoidal_positional_encoding: length {length}, E {E}")
    pos = np.arange(length, dtype=np.float64)[:, None]
    w = np.exp(np.arange(0, E, 2, dtype=np.float64) * -(np.log(10000.0) / E))[None, :]
    pe = np.empty((length, E), np.float64)
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * w), np.cos(pos * w)
    return pe


class TransformerDecoder:
    """The attention decoder of a hybrid CTC / attention model: embedding ->
    x * sqrt(E) + sinusoidal positional encoding (the toolkits'
    PositionalEncoding; asr_embed_fwd, whose rows equal embed()'s float64 host
    gather bit for bit) -> TransformerDecoderLayers -> optional final LayerNorm
    (the toolkits' after_norm) -> Linear with log-softmax (asr_linear_fwd,
    EPI_BIAS_LOGSOFTMAX).  Teacher-forced scoring of n-best lists: log_probs /
    score (asr_token_score).  Autoregressive decoding on a K/V cache: begin /
    step / prune, and beam_search / greedy on top of them
    (asr_decode_attention_fwd, asr_attn_beam_step).  embedding [V, E]; w_out
    [E, V] in the [in][out] layout, b_out [V].  A right-to-left decoder
    (reverse_weight), joint CTC / attention decoding and length penalties are
    not built."""

    def __init__(self, embedding, layers: Sequence[TransformerDecoderLayer], w_out, b_out=None,
                 final_norm: Optional[LayerNorm] = None, scale_embedding: bool = True,
                 positional_encoding: bool = True):
        self.emb = np.ascontiguousarray(embedding, dtype=np.float32)
        self.V, self.E = self.emb.shape
        self.layers = list(layers)
        if not self.layers or any(l.E != self.E for l in self.layers):
            raise ValueError("TransformerDecoder: needs at least one layer, all over the embedding's E")
        if final_norm is not None and final_norm.N != self.E:
            raise ValueError("TransformerDecoder: final_norm is not over E")
        w_out = np.asarray(w_out, np.float32)
        if w_out.shape[0] != self.E:
            raise ValueError(f"TransformerDecoder: w_out {w_out.shape} is not [E, V_out]")
        self.V_out = w_out.shape[1]
        self.w_out = DeviceMatrix.from_numpy(w_out)
        self.b_out = DeviceMatrix.from_numpy((np.zeros(self.V_out, np.float32) if b_out is None
                                              else np.asarray(b_out, np.float32)).reshape(self.V_out, 1))
        self.final_norm = final_norm
        self.emb_scale = float(np.sqrt(self.E)) if scale_embedding else 1.0
        self._emb64 = self.emb.astype(np.float64) * self.emb_scale
        self.positional_encoding = bool(positional_encoding)
        self._scratch, self._keep = _Scratch(), None
        self._emb_d, self._pe_d = None, {}

    def _emb_dev(self) -> DeviceMatrix:
        if self._emb_d is None:
            self._emb_d = DeviceMatrix.from_numpy(self.emb)
        return self._emb_d

    def _pe_dev(self, length: int):
        """The float64 positional table [length, E] on the device (None without positional encoding)."""
        if not self.positional_encoding:
            return None
        if length not in self._pe_d:
            if len(self._pe_d) >= 8:
                self._pe_d.clear()
            self._pe_d[length] = _upload(sinusoidal_positional_encoding(length, self.E))
        return self._pe_d[length]

    @classmethod
    def from_torch(cls, embedding, decoder, output, scale_embedding: bool = True,
                   positional_encoding: bool = True) -> "TransformerDecoder":
        """embedding a torch.nn.Embedding, decoder a torch.nn.TransformerDecoder
        (its .layers and optional .norm), output the torch.nn.Linear to the
        vocabulary."""
        w, b = _torch_linear(output)
        norm = getattr(decoder, "norm", None)
        return cls(embedding.weight.detach().cpu().float().numpy(),
                   [TransformerDecoderLayer.from_torch(l) for l in decoder.layers], w, b,
                   None if norm is None else LayerNorm.from_torch(norm), scale_embedding, positional_encoding)

    def embed(self, tokens: np.ndarray) -> np.ndarray:
        """float32 [U*N, E] of int tokens [U][N]: emb[token] * sqrt(E) + PE[u], on the host."""
        tokens = np.asarray(tokens)
        U, N = tokens.shape
        if tokens.size and (tokens.min() < 0 or tokens.max() >= self.V):
            raise ValueError(f"TransformerDecoder: a token outside [0, {self.V})")
        pe = (sinusoidal_positional_encoding(U, self.E) if self.positional_encoding
              else np.zeros((U, self.E), np.float64))
        x = np.empty((U, N, self.E), np.float32)
        for u in range(U):                  # one token position at a time: the float64 rows stay in cache
            x[u] = self._emb64[tokens[u]] + pe[u]
        return x.reshape(U * N, self.E)

    @staticmethod
    def _group(utt, B: int):
        """(hyp_offsets [B + 1], max_hyps) of a non-decreasing utt [N] in [0, B)."""
        ut = np.asarray(utt, np.int64)
        if ut.size and (ut.min() < 0 or ut.max() >= B or np.any(np.diff(ut) < 0)):
            raise ValueError("TransformerDecoder: utt must be non-decreasing with every value in [0, B)")
        cnt = np.bincount(ut, minlength=B)
        return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), int(max(cnt.max(), 1))

    def log_probs(self, tokens_in, lengths, utt, memory, T: int, B: int, enc_lengths=None, stream: int = 0):
        """(logp DeviceMatrix [U*N, V_out], U, N): the log-softmax outputs for
        decoder input tokens_in int [U][N] (token u of hypothesis n), of which
        lengths[n] are real; hypothesis n reads the memory [T*B, E] of utterance
        utt[n] (non-decreasing), enc_lengths[b] frames of it (None: T).  Rows
        past lengths[n] hold the log-softmax of the output bias.  logp is a
        buffer of this decoder, reused by its next call."""
        tokens_in = np.asarray(tokens_in)
        U, N = tokens_in.shape
        E, st = self.E, stream or 0
        if len(lengths) != N or len(utt) != N:
            raise ValueError(f"TransformerDecoder: {len(lengths)} lengths / {len(utt)} utt for N = {N} hypotheses")
        _need_matrix("TransformerDecoder: memory", memory, int(T) * int(B), E)
        if memory.rows != T * B or memory.cols != E:
            raise ValueError(f"TransformerDecoder: memory is {memory.rows} x {memory.cols}, not T*B x E = "
                             f"{T * B} x {E}")
        off, max_hyps = self._group(utt, B)
        ql = device_lengths(np.minimum(np.maximum(np.asarray(lengths, np.int64), 0), U))
        kl = _device_int32_exact("TransformerDecoder: enc_lengths", enc_lengths, B)
        d_off = device_lengths(off)
        sc = self._scratch                  # buffers of this decoder, reused by its next call of the same shape
        x, y, kv = sc.get("x", U * N, E), sc.get("y", U * N, E), sc.get("kv", T * B, 2 * E)
        if tokens_in.size and (tokens_in.min() < 0 or tokens_in.max() >= self.V):
            raise ValueError(f"TransformerDecoder: a token outside [0, {self.V})")
        pos = np.repeat(np.arange(U, dtype=np.int32), N) if self.positional_encoding else None
        embed_fwd(self._emb_dev(), self._pe_dev(U), np.ascontiguousarray(tokens_in, dtype=np.int32).reshape(-1), pos,
                  x, U * N, E, self.V, U, self.emb_scale, stream=st)       # embed()'s bits, gathered on the device
        for layer in self.layers:
            layer.cross_attn.project_memory(memory, T, B, out=kv, stream=st)
            layer.forward(x, U, N, kv, T, B, ql, kl, d_off, max_hyps, out=y, stream=st)
            x, y = y, x
        if self.final_norm is not None:
            self.final_norm.forward(x, U, N, ql, out=x, stream=st)
        logp = sc.get("logp", U * N, self.V_out)
        linear_fwd(x, self.w_out, self.b_out, logp, EPI_BIAS_LOGSOFTMAX, st)
        self._keep = (ql, kl, d_off)
        return logp, U, N

    @staticmethod
    def teacher_forcing(hyps: Sequence[Sequence[int]], sos: int, eos: int):
        """(tokens_in [U][N], targets [U][N], lengths [N]) int32 for hypotheses
        y: the input is sos + y, the target y + eos, U = max len(y) + 1; past a
        hypothesis's len(y) + 1 tokens both hold eos."""
        N = len(hyps)
        U = max([len(y) for y in hyps] + [0]) + 1
        tin, tgt = np.full((U, N), eos, np.int32), np.full((U, N), eos, np.int32)
        for n, y in enumerate(hyps):
            tin[0, n] = sos
            tin[1:len(y) + 1, n] = y
            tgt[:len(y), n] = y
        return tin, tgt, np.array([len(y) + 1 for y in hyps], np.int32)

    def score(self, hyps: Sequence[Sequence[int]], utt: Sequence[int], memory, T: int, B: int, enc_lengths=None,
              sos: Optional[int] = None, eos: Optional[int] = None, stream: int = 0) -> np.ndarray:
        """The attention log-likelihood of every hypothesis, fp64 [N]: the sum of
        log p(y_u | sos, y_<u, memory of utt[n]) over y + eos (len(y) + 1 terms).
        utt non-decreasing; sos / eos default to V - 1 (the toolkits' shared
        <sos/eos>).  The [U*N, V] log-probs stay on the device."""
        sos = self.V - 1 if sos is None else int(sos)
        eos = self.V - 1 if eos is None else int(eos)
        if not len(hyps):
            return np.zeros(0, np.float64)
        tin, tgt, ln = self.teacher_forcing(hyps, sos, eos)
        logp, U, N = self.log_probs(tin, ln, utt, memory, T, B, enc_lengths, stream)
        return token_score(logp, tgt, ln, U, N, self.V_out, stream=stream or 0)

    # ------------------------------------------------ autoregressive decoding
    def begin(self, memory, T: int, B: int, enc_lengths=None, beam: int = 10, max_len: Optional[int] = None,
              sos: Optional[int] = None, stream: int = 0) -> "DecoderState":
        """Start a search over memory [T*B, E] (row j*B + b: frame j of
        utterance b; enc_lengths[b] frames of it, None: T) with beam slots per
        utterance, slot n = b*beam + k, and at most max_len (default T) steps:
        the DecoderState with the per-layer K/V caches [max_len*N, 3E], the
        per-layer projected memory (project_memory runs here, once per
        search), the ancestry and token tables, the scores (slot k = 0 of each
        utterance 0, the others -inf) and flags, and the utterances' slot
        offsets and encoder lengths."""
        T, B, K, E = int(T), int(B), int(beam), self.E
        max_len = T if max_len is None else int(max_len)
        sos = self.V - 1 if sos is None else int(sos)
        if T < 1 or B < 1 or max_len < 1:
            raise ValueError(f"TransformerDecoder.begin: T {T}, B {B}, max_len {max_len}")
        if K < 1 or K > ATTN_BEAM_MAX_K:
            raise ValueError(f"TransformerDecoder.begin: beam {K} outside [1, {ATTN_BEAM_MAX_K}]")
        if sos < 0 or sos >= self.V:
            raise ValueError(f"TransformerDecoder.begin: sos {sos} outside [0, {self.V})")
        if self.V_out > self.V:
            raise ValueError(f"TransformerDecoder.begin: {self.V_out} outputs cannot be fed back into an embedding "
                             f"of {self.V} rows")
        _need_matrix("TransformerDecoder.begin: memory", memory, T * B, E)
        if memory.rows != T * B or memory.cols != E:
            raise ValueError(f"TransformerDecoder.begin: memory is {memory.rows} x {memory.cols}, not T*B x E = "
                             f"{T * B} x {E}")
        if enc_lengths is None:
            enc = np.full(B, T, np.int32)
        elif isinstance(enc_lengths, DeviceBytes):
            _need_int32("TransformerDecoder.begin: enc_lengths", enc_lengths, B)
            enc = None
        else:
            if len(enc_lengths) != B:
                raise ValueError(f"TransformerDecoder.begin: {len(enc_lengths)} enc_lengths, not B = {B}")
            enc = np.asarray(enc_lengths, np.int64)
        if enc is None:
            enc = device_int32(enc_lengths, B, stream or 0)
        enc = np.minimum(np.maximum(enc, 0), T).astype(np.int32)
        return DecoderState(self, memory, T, B, K, max_len, sos, enc, stream or 0)

    def step(self, state: "DecoderState", tokens=None, parents=None, stream: int = 0) -> DeviceMatrix:
        """One decoder step for every slot from the state's current tokens (sos
        at step 0): the log-probs [N, V_out] on the device (a buffer of the
        state, reused by the next step).  After step s the caller decides the
        tokens of step s: prune() on the device, or tokens [N] and parents [N]
        given to the NEXT step() call (slot n then continues slot parents[n],
        a slot of its own utterance, with tokens[n]): the caller drives the
        reorder, and the tables are permuted on the host."""
        N, E, st = state.N, self.E, stream or 0
        s = state.steps
        if state.decoder is not self:
            raise ValueError("TransformerDecoder.step: the state belongs to another decoder")
        if s >= state.max_len:
            raise ValueError(f"TransformerDecoder.step: the state's max_len = {state.max_len} steps are used up")
        if (tokens is None) != (parents is None):
            raise ValueError("TransformerDecoder.step: tokens and parents come together")
        if tokens is not None:
            if s == 0 or state.decided != s - 1:
                raise ValueError("TransformerDecoder.step: tokens / parents decide a step that has run and has "
                                 "not been decided")
            tk, pa = np.asarray(tokens), np.asarray(parents)
            if tk.shape != (N,) or pa.shape != (N,):
                raise ValueError(f"TransformerDecoder.step: tokens {tk.shape} / parents {pa.shape}, not ({N},)")
            if tk.min() < 0 or tk.max() >= self.V:
                raise ValueError(f"TransformerDecoder.step: a token outside [0, {self.V})")
            if pa.min() < 0 or pa.max() >= N or np.any(pa // state.K != np.arange(N) // state.K):
                raise ValueError("TransformerDecoder.step: a parent outside its slot's utterance")
            state._reorder_host(tk.astype(np.int32), pa.astype(np.int64), st)
        elif state.decided != s:
            raise ValueError(f"TransformerDecoder.step: the tokens of step {s - 1} are not decided: prune() or give "
                             "tokens / parents")
        tok = state.sos if s == 0 else Int32View(state.tok[state.cur], (s - 1) * N, N)
        pos = Int32View(state.pos, s * N, N) if self.positional_encoding else None
        x, y = state.x, state.y
        embed_fwd(self._emb_dev(), state.pe, tok, pos, x, N, E, self.V, state.max_len, self.emb_scale, stream=st)
        for layer, cache, kv in zip(self.layers, state.caches, state.kvs):
            layer.step(x, N, cache, s, state.anc[state.cur], kv, state.T, state.B, state.off, state.K, state.klen,
                       out=y, stream=st)
            x, y = y, x
        if self.final_norm is not None:
            self.final_norm.forward(x, 1, N, None, out=x, stream=st)
        linear_fwd(x, self.w_out, self.b_out, state.logp, EPI_BIAS_LOGSOFTMAX, st)
        state.steps = s + 1
        return state.logp

    def prune(self, state: "DecoderState", logp=None, eos: Optional[int] = None, stream: int = 0) -> int:
        """Decide the step that has just run on the device (asr_attn_beam_step
        on logp, default the state's): scores, flags, tokens and both tables.
        Returns the number of live unfinished slots, one 4-byte read, EVERY
        step: the read costs one synchronisation of a loop that is otherwise
        queued ahead, and ends the search at the step the last hypothesis
        ends."""
        eos = self.V - 1 if eos is None else int(eos)
        s, st = state.steps - 1, stream or 0
        if s < 0 or state.decided != s:
            raise ValueError("TransformerDecoder.prune: no step has run that is not decided")
        if eos < 0 or eos >= self.V_out:
            raise ValueError(f"TransformerDecoder.prune: eos {eos} outside [0, {self.V_out})")
        logp = state.logp if logp is None else logp
        c, o = state.cur, 1 - state.cur
        attn_beam_step(attn_beam_desc(state.B, state.K, self.V_out, state.max_len, s, eos), logp, state.scores[c],
                       state.fin[c], state.tok[c], state.anc[c], state.scores[o], state.fin[o], state.parent,
                       state.token, state.tok[o], state.anc[o], state.live, stream=st)
        state.cur, state.decided, state.eos = o, s + 1, eos
        return int(device_int32(state.live, 1, st)[0])

    def beam_search(self, memory, T: int, B: int, enc_lengths=None, beam: int = 10, max_len: Optional[int] = None,
                    sos: Optional[int] = None, eos: Optional[int] = None, nbest: Optional[int] = None,
                    stream: int = 0):
        """Attention-decoder beam search (the toolkits' `attention` decode
        mode): per utterance [(tokens, score)], score descending (equal scores
        in slot order), tokens without sos / eos, at most nbest (default beam)
        of them; score is the float64 sum of the chosen tokens' fp32 log-probs,
        eos included.  A finished hypothesis stays in the beam with its score
        (WeNet's masking); the loop ends when no live unfinished slot is left
        (prune()'s count, read every step) or after max_len (default T) steps,
        and hypotheses that have not ended by then are returned as they stand.
        An utterance with no encoder frames returns [([], score)], score the
        log-prob of eos after sos over an all-zero context.  The result plugs
        into attention_combine, nbest_mbr and edit_distance as the other
        searches' n-bests do."""
        eos = self.V - 1 if eos is None else int(eos)
        if eos < 0 or eos >= self.V_out:
            raise ValueError(f"TransformerDecoder.beam_search: eos {eos} outside [0, {self.V_out})")
        if nbest is not None and nbest < 1:
            raise ValueError(f"TransformerDecoder.beam_search: nbest {nbest}")
        state = self.begin(memory, T, B, enc_lengths, beam, max_len, sos, stream)
        empty, none = {}, np.flatnonzero(state.enc == 0)
        for s in range(state.max_len):
            logp = self.step(state, stream=stream)
            if s == 0:                       # an utterance without frames: its result is this step's eos
                one = np.empty(1, np.float32)
                for b in none:
                    check(lib().asr_memcpy_d2h(_ptr(one), logp.ptr + 4 * (int(b) * state.K * logp.cols + eos), 4,
                                               stream or 0), "asr_memcpy_d2h")
                    empty[int(b)] = float(np.float64(one[0]))
            live = self.prune(state, logp, eos, stream)
            if s == 0 and len(none):         # ... and its slots leave the search: they hold no one up
                state.drop_utterances(none, stream or 0)
                live = 1
            if live == 0:
                break
        out = state.results(nbest)
        for b, sc in empty.items():
            out[b] = [([], sc)]
        return out

    def greedy(self, memory, T: int, B: int, enc_lengths=None, max_len: Optional[int] = None,
               sos: Optional[int] = None, eos: Optional[int] = None, stream: int = 0):
        """beam_search with one slot per utterance."""
        return self.beam_search(memory, T, B, enc_lengths, 1, max_len, sos, eos, None, stream)


class DecoderState:
    """The state of one autoregressive search of a TransformerDecoder
    (TransformerDecoder.begin): N = B*K slots, slot n = b*K + k.  On the
    device: caches[l] [max_len*N, 3E] (row j*N + n: the Q / K / V row slot n
    wrote at step j), kvs[l] [T*B, 2E] the projected memory of layer l, the
    ancestry and token tables anc / tok (int32 [max_len][N], two copies each:
    a prune gathers from one into the other), scores (fp64 [N]) and fin (int32
    [N]) likewise, off / klen (the slots of each utterance, [B + 1], and its encoder frames, [B]),
    parent / token of the last prune and the live count.  steps: decoder steps
    run; decided: steps whose tokens are decided."""

    def __init__(self, decoder, memory, T, B, K, max_len, sos, enc, stream=0):
        N, E = B * K, decoder.E
        self.decoder, self.T, self.B, self.K, self.N, self.max_len = decoder, T, B, K, N, max_len
        self.steps, self.decided, self.cur, self.eos, self.enc = 0, 0, 0, None, enc
        self.caches = [DeviceMatrix(max_len * N, 3 * E) for _ in decoder.layers]
        self.kvs = [l.cross_attn.project_memory(memory, T, B, stream=stream) for l in decoder.layers]
        ident = np.tile(np.arange(N, dtype=np.int32), (max_len, 1))
        self.anc = [_upload(ident, stream), _upload(ident, stream)]
        zeros = np.zeros((max_len, N), np.int32)
        self.tok = [_upload(zeros, stream), _upload(zeros, stream)]
        sc = np.full(N, -np.inf, np.float64)
        sc[::K] = 0.0
        self.scores = [_upload(sc, stream), _upload(sc, stream)]
        self.fin = [_upload(np.zeros(N, np.int32), stream), _upload(np.zeros(N, np.int32), stream)]
        self.off = _upload(np.arange(B + 1, dtype=np.int32) * K, stream)
        self.klen = _upload(enc.astype(np.int32), stream)
        self.pos = _upload(np.repeat(np.arange(max_len, dtype=np.int32), N), stream)
        self.sos = _upload(np.full(N, sos, np.int32), stream)
        self.pe = decoder._pe_dev(max_len)
        self.parent, self.token, self.live = DeviceBytes(4 * N), DeviceBytes(4 * N), DeviceBytes(16)
        self.x, self.y = DeviceMatrix(N, E), DeviceMatrix(N, E)
        self.logp = DeviceMatrix(N, decoder.V_out)

    def _reorder_host(self, tokens, parents, stream=0):
        """The caller's decision of step steps - 1: both tables through parents, on the host."""
        N, L, s, c = self.N, self.max_len, self.steps - 1, self.cur
        tok = _download(self.tok[c], (L, N), np.int32, stream)
        anc = _download(self.anc[c], (L, N), np.int32, stream)
        tok[:s] = tok[:s, parents]
        tok[s] = tokens
        anc[:s + 1] = anc[:s + 1, parents]
        if s + 1 < L:
            anc[s + 1] = np.arange(N, dtype=np.int32)
        for d, a in ((self.tok[c], tok), (self.anc[c], anc)):
            check(lib().asr_memcpy_h2d(d.ptr, _ptr(a), a.nbytes, stream), "asr_memcpy_h2d")
        self.decided = s + 1

    def drop_utterances(self, utts, stream=0):
        """Empty every slot of the given utterances (score -inf): the next prune finds no candidate there."""
        gone = np.full(self.K, -np.inf, np.float64)
        for b in utts:
            check(lib().asr_memcpy_h2d(self.scores[self.cur].ptr + 8 * int(b) * self.K, _ptr(gone), gone.nbytes,
                                       stream), "asr_memcpy_h2d")

    def tables(self, stream=0):
        """(tokens [decided][N], ancestry [steps..][N], scores [N], finished [N]) on the host."""
        N, L, c = self.N, self.max_len, self.cur
        return (_download(self.tok[c], (L, N), np.int32, stream)[:self.decided],
                _download(self.anc[c], (L, N), np.int32, stream)[:min(self.decided + 1, L)],
                _download(self.scores[c], N, np.float64, stream), _download(self.fin[c], N, np.int32, stream))

    def results(self, nbest=None, stream=0):
        """Per utterance [(tokens, score)] of the live slots, score descending,
        tokens cut before the first eos of the last prune."""
        tok, _anc, sc, _fin = self.tables(stream)
        out = []
        for b in range(self.B):
            rows = []
            for n in range(b * self.K, (b + 1) * self.K):
                if not sc[n] > -np.inf:
                    continue
                y = tok[:, n].tolist()
                if self.eos is not None and self.eos in y:
                    y = y[:y.index(self.eos)]
                rows.append((y, float(sc[n])))
            rows.sort(key=lambda r: -r[1])
            out.append(rows[:nbest] if nbest is not None else rows)
        return out


def attention_combine(nbest, att, ctc, ctc_weight: float):
    """Per utterance [(labels, total, att, exact_ctc)] with total = att +
    ctc_weight * exact_ctc, total descending, equal totals in their beam order
    (a stable sort); att and ctc are flat over the hypotheses in nbest's order.
    Host only."""
    out, k = [], 0
    for u in nbest:
        rows = [(list(h[0]), float(att[k + j]) + ctc_weight * float(ctc[k + j]), float(att[k + j]),
                 float(ctc[k + j])) for j, h in enumerate(u)]
        k += len(u)
        out.append(sorted(rows, key=lambda r: -r[1]))
    return out


def attention_rescore(nbest, decoder: TransformerDecoder, memory, T: int, B: int, enc_lengths=None,
                      ctc_scores=None, ctc_weight: float = 0.5, sos: Optional[int] = None,
                      eos: Optional[int] = None, stream: int = 0):
    """Attention-decoder rescoring of an n-best (WeNet's attention_rescoring,
    ESPnet's joint CTC / attention score): per utterance [(labels, total, att,
    exact_ctc)], total = att + ctc_weight * exact_ctc descending, equal totals
    in their beam order; an utterance with an empty beam gives [].  nbest: per
    utterance a list of hypotheses whose first element is the label list
    (CTCDecoder.beams / rescore, TransducerDecoder.beam_search); ctc_scores:
    per utterance the first-pass score of each hypothesis (None: each
    hypothesis's own second element).  memory [T*B, E] is the encoder output on
    the device, enc_lengths its frames per utterance."""
    if len(nbest) != B:
        raise ValueError(f"attention_rescore: {len(nbest)} n-best lists for B = {B} utterances")
    if ctc_scores is None:
        ctc_scores = [[h[1] for h in u] for u in nbest]
    if len(ctc_scores) != B or any(len(c) != len(u) for c, u in zip(ctc_scores, nbest)):
        raise ValueError("attention_rescore: ctc_scores does not match the n-best")
    hyps = [list(h[0]) for u in nbest for h in u]
    if not hyps:
        return [[] for _ in nbest]
    utt = [b for b, u in enumerate(nbest) for _ in u]
    att = decoder.score(hyps, utt, memory, T, B, enc_lengths, sos, eos, stream)
    return attention_combine(nbest, att, [c for u in ctc_scores for c in u], ctc_weight)


# ------------------------------------------------------------------ Conformer
GLU_ACT_NONE, GLU_ACT_RELU, GLU_ACT_SILU = 0, 1, 2
GLU_ACTS = {None: GLU_ACT_NONE, "none": GLU_ACT_NONE, "relu": GLU_ACT_RELU, "silu": GLU_ACT_SILU,
            "swish": GLU_ACT_SILU}
GLU_DWCONV_MAX_KERNEL = 80   # ASR_GLU_DWCONV_MAX_KERNEL


class GluDwconvDesc(ctypes.Structure):
    """asr_glu_dwconv_desc (include/asr_amd.h)."""
    _fields_ = [("channels", _i), ("kernel", _i), ("pad_left", _i), ("pad_right", _i), ("act", _i)]


def glu_dwconv_desc(channels: int, kernel: int, pad_left: Optional[int] = None, pad_right: Optional[int] = None,
                    act="silu") -> GluDwconvDesc:
    """A GluDwconvDesc from keywords; the pads default to "same"
    ((k-1)//2, k-1 - (k-1)//2); act: None, "relu", "silu" or an ASR_GLU_ACT_* value."""
    if pad_left is None:
        pad_left = (kernel - 1) // 2 if pad_right is None else kernel - 1 - pad_right
    if pad_right is None:
        pad_right = kernel - 1 - pad_left
    a = GLU_ACTS[act.lower()] if isinstance(act, str) else GLU_ACT_NONE if act is None else int(act)
    return GluDwconvDesc(channels, kernel, pad_left, pad_right, a)


def glu_dwconv_fwd(u, w: DeviceMatrix, b: Optional[DeviceMatrix], out, T: int, B: int, desc: GluDwconvDesc,
                   lengths: Optional[DeviceBytes] = None, col: int = 0, stream: int = 0):
    """GLU -> depthwise convolution over time -> bias -> activation in one
    launch (asr_glu_dwconv_fwd): u [T*B, >= 2C] time-major, values in columns
    [0, C) and gates in [C, 2C) (the row stride is u.cols), w [k, C], b [C] or
    None, the result into columns [col, col + C) of out [T*B, >= C] (the row
    stride is out.cols); lengths from device_lengths()."""
    C = desc.channels
    assert u.rows == T * B and u.cols >= 2 * C, (u.rows, u.cols)
    assert out.rows == T * B, (out.rows, T, B)
    assert 0 <= col and col + C <= out.cols, (out.cols, col)
    assert w.rows * w.cols == desc.kernel * C, (w.rows, w.cols)
    opt = lambda m: m.ptr if m is not None else None   # noqa: E731
    check(lib().asr_glu_dwconv_fwd(ctypes.byref(desc), u.ptr, u.cols, opt(lengths), w.ptr, opt(b),
                                   out.ptr + 4 * col, out.cols, T, B, stream), "asr_glu_dwconv_fwd")
    return out


def _torch_linear(lin):
    """(W [in][out], b [out]) float32 of a torch.nn.Linear."""
    host = lambda p: p.detach().cpu().float().numpy()   # noqa: E731
    b = host(lin.bias) if lin.bias is not None else np.zeros(lin.out_features, np.float32)
    return np.ascontiguousarray(host(lin.weight).T), b


class ConformerConv:
    """The convolution module of a Conformer block for inference, time-major:
    LayerNorm -> pointwise conv to 2E -> GLU -> depthwise conv -> BatchNorm ->
    SiLU -> pointwise conv to E, as asr_layernorm_fwd, asr_linear_fwd,
    asr_glu_dwconv_fwd (the eval-mode BatchNorm folded into its weights and
    bias) and asr_linear_fwd.  No arithmetic here.  w1 [E, 2E], wd [k, E] and
    w2 [E, E] in this library's [in][out] / [tap][channel] layouts; padding
    'same', 'causal' or (left, right) with left + right = k - 1."""

    def __init__(self, norm: LayerNorm, w1, b1, wd, bd, w2, b2, padding="same", act="silu"):
        E = norm.N
        wd = np.asarray(wd, np.float32)
        k = wd.shape[0]
        assert wd.shape == (k, E), wd.shape
        pl, pr = Conv1d.parse_padding(padding, k)
        self.E, self.norm = E, norm
        self.desc = glu_dwconv_desc(E, k, pl, pr, act)
        up = lambda a, shape: DeviceMatrix.from_numpy(np.asarray(a, np.float32).reshape(shape))   # noqa: E731
        self.w1, self.b1 = up(w1, (E, 2 * E)), up(b1, (2 * E, 1))
        self.wd, self.bd = up(wd, (k, E)), up(bd, (E, 1))
        self.w2, self.b2 = up(w2, (E, E)), up(b2, (E, 1))
        self._scratch, self._keep = _Scratch(), None

    @staticmethod
    def pack_torch(norm, pw1, dw, bn, pw2, padding=None):
        """A dict of float32 arrays and the padding from the five torch
        modules of a convolution module: w1 [E, 2E] / b1 and w2 [E, E] / b2
        (the 1x1 Conv1d weights transposed to [in][out]), wd [k, E] / bd (the
        depthwise weights with the eval-mode BatchNorm1d folded in float64, as
        Conv1d.pack_torch does, rounded to fp32 once), 'padding': (left,
        right) from dw.padding, or from the padding argument ((left, right) or
        'causal') when dw.padding is 0 (models that pad by hand), and the
        LayerNorm's 'norm_weight' / 'norm_bias' / 'norm_eps'.  No device call.
        Raises ValueError for a GroupNorm / LayerNorm in place of the BatchNorm,
        a BatchNorm in training mode or without running statistics,
        dw.groups != channels, a stride or dilation other than 1, a pointwise
        kernel size other than 1, or pads that do not sum to k - 1."""
        E = dw.in_channels
        if not hasattr(bn, "running_mean") or not hasattr(bn, "running_var"):
            raise ValueError(f"ConformerConv.pack_torch: {type(bn).__name__} in place of the BatchNorm1d is not "
                             "supported")
        if dw.groups != E or dw.out_channels != E:
            raise ValueError("ConformerConv.pack_torch: the depthwise convolution needs groups == channels")
        if dw.stride[0] != 1 or dw.dilation[0] != 1:
            raise ValueError("ConformerConv.pack_torch: the depthwise convolution needs stride 1 and dilation 1")
        for name, pw, cout in (("first", pw1, 2 * E), ("second", pw2, E)):
            if pw.kernel_size[0] != 1 or pw.stride[0] != 1 or pw.groups != 1 or pw.padding not in ((0,), "valid"):
                raise ValueError(f"ConformerConv.pack_torch: the {name} pointwise convolution needs kernel size 1, "
                                 "stride 1, no padding and groups 1")
            if pw.in_channels != E or pw.out_channels != cout:
                raise ValueError(f"ConformerConv.pack_torch: the {name} pointwise convolution is "
                                 f"{pw.in_channels} -> {pw.out_channels}, not {E} -> {cout}")
        if tuple(norm.normalized_shape) != (E,):
            raise ValueError(f"ConformerConv.pack_torch: LayerNorm over {tuple(norm.normalized_shape)}, not ({E},)")
        wd, bd, kw = Conv1d.pack_torch(dw, bn)          # refuses a BatchNorm in training mode; folds in float64
        k = kw["kernel"]
        pads = kw["padding"]
        if padding is not None:
            if pads != (0, 0):
                raise ValueError("ConformerConv.pack_torch: a padding argument needs dw.padding == 0")
            pads = Conv1d.parse_padding(padding, k)
        if pads[0] < 0 or pads[1] < 0 or pads[0] + pads[1] != k - 1:
            raise ValueError(f"ConformerConv.pack_torch: pads {pads} do not sum to kernel - 1 = {k - 1}")
        host = lambda p: p.detach().cpu().float().numpy()   # noqa: E731
        pwb = lambda pw: (host(pw.bias) if pw.bias is not None   # noqa: E731
                          else np.zeros(pw.out_channels, np.float32))
        return dict(w1=np.ascontiguousarray(host(pw1.weight)[:, :, 0].T), b1=pwb(pw1), wd=wd.reshape(k, E), bd=bd,
                    w2=np.ascontiguousarray(host(pw2.weight)[:, :, 0].T), b2=pwb(pw2), padding=pads,
                    norm_weight=None if getattr(norm, "weight", None) is None else host(norm.weight),
                    norm_bias=None if getattr(norm, "bias", None) is None else host(norm.bias),
                    norm_eps=float(norm.eps))

    @classmethod
    def _from_packed(cls, p) -> "ConformerConv":
        norm = LayerNorm(p["w2"].shape[0], p["norm_eps"], p["norm_weight"], p["norm_bias"])
        return cls(norm, p["w1"], p["b1"], p["wd"], p["bd"], p["w2"], p["b2"], padding=p["padding"])

    @classmethod
    def from_torch(cls, norm, pw1, dw, bn, pw2, padding=None) -> "ConformerConv":
        return cls._from_packed(cls.pack_torch(norm, pw1, dw, bn, pw2, padding))

    def forward(self, x, T: int, B: int, lengths=None, out=None, zero_padding: bool = True, stream: int = 0):
        """The module (without its residual) of time-major x [T*B, E]; lengths
        None, a sequence of B counts or a DeviceBytes of int32 [B]: frames past
        them are zero padding for the convolution whatever x holds.  Returns
        out [T*B, E] (a buffer of this module, reused by its next call, unless
        given); rows past the lengths are zeros unless zero_padding is False,
        in which case they hold the last bias."""
        E, M, st = self.E, T * B, stream or 0
        lengths = _device_lengths_or_none(lengths)
        sc = self._scratch
        n, u, c = sc.get("n", M, E), sc.get("u", M, 2 * E), sc.get("c", M, E)
        out = sc.get("out", M, E) if out is None else out
        self.norm.forward(x, T, B, lengths, out=n, stream=st)
        linear_fwd(n, self.w1, self.b1, u, EPI_BIAS, st)
        glu_dwconv_fwd(u, self.wd, self.bd, c, T, B, self.desc, lengths=lengths, stream=st)
        linear_fwd(c, self.w2, self.b2, out, EPI_BIAS, st)
        if zero_padding and lengths is not None:
            mask_rows(out, T, B, E, lengths, st)
        self._keep = lengths
        return out


class ConformerLayer:
    """One Conformer encoder block for inference, time-major:
        x + 1/2 FFN1(x) -> attention and convolution module, each with its
        residual (the convolution first if convolution_first) -> + 1/2 FFN2 ->
        LayerNorm,
    each FFN LayerNorm -> Linear -> SiLU -> Linear.  The feed-forwards are
    asr_linear_fwd with EPI_BIAS_SILU and EPI_BIAS, the 1/2 folded into the second
    linear's weights and bias when packing (exact: a power of two); attention
    is MultiheadAttention (with its chunk / left / right window), the
    convolution module ConformerConv; the residuals are asr_matadd, the last one
    the fused residual of the final asr_layernorm_fwd.  No arithmetic here;
    dropout is ignored.  ffn1 / ffn2: (LayerNorm, w1 [E, F], b1 [F], w2 [F, E],
    b2 [E]) with w2 and b2 already halved (pack_ffn)."""

    def __init__(self, ffn1, attn_norm: LayerNorm, attn: MultiheadAttention, conv: ConformerConv, ffn2,
                 final_norm: LayerNorm, convolution_first: bool = False):
        E = attn.E
        assert conv.E == E and attn_norm.N == E and final_norm.N == E, (E, conv.E, attn_norm.N, final_norm.N)
        self.E, self.convolution_first = E, bool(convolution_first)
        self.attn_norm, self.attn, self.conv, self.final_norm = attn_norm, attn, conv, final_norm
        self.ffn = []
        for ln, w1, b1, w2, b2 in (ffn1, ffn2):
            w1, w2 = np.asarray(w1, np.float32), np.asarray(w2, np.float32)
            F = w1.shape[1]
            assert ln.N == E and w1.shape == (E, F) and w2.shape == (F, E), (ln.N, w1.shape, w2.shape)
            self.ffn.append((ln, F, DeviceMatrix.from_numpy(w1),
                             DeviceMatrix.from_numpy(np.asarray(b1, np.float32).reshape(F, 1)),
                             DeviceMatrix.from_numpy(w2),
                             DeviceMatrix.from_numpy(np.asarray(b2, np.float32).reshape(E, 1))))
        self._scratch, self._keep = _Scratch(), None

    @staticmethod
    def pack_ffn(ln, lin1, lin2):
        """(w1 [E, F], b1 [F], w2 / 2 [F, E], b2 / 2 [E]) float32 of a
        feed-forward module LayerNorm -> lin1 -> SiLU -> lin2 whose output the
        block halves: the 1/2 goes into lin2 (a multiplication by a power of
        two commutes with every fp32 rounding).  No device call."""
        w1, b1 = _torch_linear(lin1)
        w2, b2 = _torch_linear(lin2)
        if lin2.in_features != lin1.out_features or lin1.in_features != lin2.out_features:
            raise ValueError("ConformerLayer.pack_ffn: the two linears do not chain E -> F -> E")
        return w1, b1, np.float32(0.5) * w2, np.float32(0.5) * b2

    @staticmethod
    def pack_torch(ffn1, attn, conv, ffn2, final_norm, conv_padding=None):
        """Every packed float32 array of a block, from its torch parts (the
        arguments of from_torch): a flat dict 'ffn1.w1', ..., 'attn.w_in', ...,
        'conv.wd', ..., and the LayerNorms' '<part>.norm_weight' / '.norm_bias'
        / '.norm_eps'.  No device call."""
        host = lambda p: None if p is None else p.detach().cpu().float().numpy()   # noqa: E731
        out = {}

        def norm(prefix, ln):
            if len(tuple(ln.normalized_shape)) != 1:
                raise ValueError(f"ConformerLayer.pack_torch: {prefix} LayerNorm over {tuple(ln.normalized_shape)}")
            out[prefix + ".norm_weight"] = host(getattr(ln, "weight", None))
            out[prefix + ".norm_bias"] = host(getattr(ln, "bias", None))
            out[prefix + ".norm_eps"] = float(ln.eps)

        for name, (ln, lin1, lin2) in (("ffn1", ffn1), ("ffn2", ffn2)):
            norm(name, ln)
            for key, a in zip(("w1", "b1", "w2", "b2"), ConformerLayer.pack_ffn(ln, lin1, lin2)):
                out[f"{name}.{key}"] = a
        norm("attn", attn[0])
        for key, a in zip(("w_in", "b_in", "w_out", "b_out"), MultiheadAttention.pack_torch(attn[1])):
            out["attn." + key] = a
        out["attn.heads"] = int(attn[1].num_heads)
        for key, a in ConformerConv.pack_torch(*conv, padding=conv_padding).items():
            out["conv." + key] = a
        norm("final", final_norm)
        return out

    @classmethod
    def from_torch(cls, ffn1, attn, conv, ffn2, final_norm, convolution_first: bool = False, chunk: int = 1,
                   left: int = -1, right: int = -1, conv_padding=None) -> "ConformerLayer":
        """From explicit torch parts: ffn1 / ffn2 = (LayerNorm, Linear, Linear),
        attn = (LayerNorm, MultiheadAttention), conv = (LayerNorm, pointwise
        Conv1d, depthwise Conv1d, BatchNorm1d, pointwise Conv1d), final_norm a
        LayerNorm; chunk / left / right the attention window; conv_padding as
        ConformerConv.pack_torch's padding."""
        p = cls.pack_torch(ffn1, attn, conv, ffn2, final_norm, conv_padding)
        E = p["attn.w_out"].shape[0]
        ln = lambda k: LayerNorm(E, p[k + ".norm_eps"], p[k + ".norm_weight"], p[k + ".norm_bias"])   # noqa: E731
        ffn = lambda k: (ln(k), p[k + ".w1"], p[k + ".b1"], p[k + ".w2"], p[k + ".b2"])   # noqa: E731
        mha = MultiheadAttention(E, p["attn.heads"], p["attn.w_in"], p["attn.b_in"], p["attn.w_out"],
                                 p["attn.b_out"], chunk, left, right)
        conv_m = ConformerConv._from_packed({k[5:]: v for k, v in p.items() if k.startswith("conv.")})
        return cls(ffn("ffn1"), ln("attn"), mha, conv_m, ffn("ffn2"), ln("final"), convolution_first)

    @staticmethod
    def torchaudio_parts(layer) -> dict:
        """The parts of from_torch read off a module laid out like
        torchaudio.models.conformer.ConformerLayer (see from_torchaudio)."""
        f1, f2, cm = layer.ffn1.sequential, layer.ffn2.sequential, layer.conv_module
        return dict(ffn1=(f1[0], f1[1], f1[4]), attn=(layer.self_attn_layer_norm, layer.self_attn),
                    conv=(cm.layer_norm, cm.sequential[0], cm.sequential[2], cm.sequential[3], cm.sequential[5]),
                    ffn2=(f2[0], f2[1], f2[4]), final_norm=layer.final_layer_norm,
                    convolution_first=bool(layer.convolution_first))

    @classmethod
    def from_torchaudio(cls, layer, chunk: int = 1, left: int = -1, right: int = -1,
                        conv_padding=None) -> "ConformerLayer":
        """A thin adapter over from_torch for a module with the attribute
        layout of torchaudio's ConformerLayer: ffn1.sequential[0, 1, 4]
        (LayerNorm, Linear, Linear), self_attn_layer_norm, self_attn,
        conv_module.layer_norm, conv_module.sequential[0, 2, 3, 5] (pointwise,
        depthwise, BatchNorm1d, pointwise), ffn2, final_layer_norm,
        convolution_first.  That layout is written from memory: this adapter
        was never run against torchaudio itself, only against a stand-in
        module with those attribute names (tests/conformer_reference.py).  A
        layer built with use_group_norm=True is refused by
        ConformerConv.pack_torch."""
        return cls.from_torch(**cls.torchaudio_parts(layer), chunk=chunk, left=left, right=right,
                              conv_padding=conv_padding)

    def _ffn(self, i: int, x, T: int, B: int, lengths, st: int):
        """FFN_i(x) / 2 into a scratch buffer."""
        ln, F, w1, b1, w2, b2 = self.ffn[i]
        M, sc = T * B, self._scratch
        n, ff, t = sc.get("n", M, self.E), sc.get("ff", M, F), sc.get("t", M, self.E)
        ln.forward(x, T, B, lengths, out=n, stream=st)
        linear_fwd(n, w1, b1, ff, EPI_BIAS_SILU, st)
        linear_fwd(ff, w2, b2, t, EPI_BIAS, st)
        return t

    def forward(self, x, T: int, B: int, lengths=None, stream: int = 0) -> DeviceMatrix:
        """x time-major [T*B, E]; lengths None, a sequence of B counts or a
        DeviceBytes of int32 [B] (e.g. Conv1d.forward's out_lengths).  Returns a
        new DeviceMatrix [T*B, E] with zero rows past the lengths; rows of x
        past them may hold anything."""
        E, M, st = self.E, T * B, stream or 0
        lengths = _device_lengths_or_none(lengths)
        sc = self._scratch
        h, h2, n = sc.get("h", M, E), sc.get("h2", M, E), sc.get("n", M, E)
        add = lambda a, b, z: check(lib().asr_matadd(a.ptr, b.ptr, z.ptr, M, E, 1.0, st), "asr_matadd")   # noqa: E731
        out = DeviceMatrix(M, E)
        add(x, self._ffn(0, x, T, B, lengths, st), h)
        for module in ("conv", "attn") if self.convolution_first else ("attn", "conv"):
            if module == "attn":
                self.attn_norm.forward(h, T, B, lengths, out=n, stream=st)
                r = self.attn.forward(n, T, B, lengths, zero_padding=False, stream=st)
            else:
                r = self.conv.forward(h, T, B, lengths, zero_padding=False, stream=st)
            add(h, r, h2)
            h, h2 = h2, h
        t = self._ffn(1, h, T, B, lengths, st)
        self.final_norm.forward(t, T, B, lengths, res=h, out=out, stream=st)
        self._keep = lengths
        return out


class Conformer:
    """A stack of ConformerLayers run in turn with the same lengths."""

    def __init__(self, layers: Sequence[ConformerLayer]):
        self.layers = list(layers)
        assert self.layers and all(l.E == self.layers[0].E for l in self.layers)
        self.E = self.layers[0].E

    def forward(self, x, T: int, B: int, lengths=None, stream: int = 0) -> DeviceMatrix:
        """x time-major [T*B, E]; returns the last layer's new DeviceMatrix
        [T*B, E] with zero rows past the lengths."""
        lengths = _device_lengths_or_none(lengths)
        for layer in self.layers:
            x = layer.forward(x, T, B, lengths, stream=stream)
        self._keep = lengths
        return x


# ----------------------------------------------------------------- front end
FBANK_WIN_HANN, FBANK_WIN_HAMMING, FBANK_WIN_RECT = 0, 1, 2
FBANK_WINDOWS = {"hann": FBANK_WIN_HANN, "hamming": FBANK_WIN_HAMMING, "rect": FBANK_WIN_RECT}


class FbankConfig(ctypes.Structure):
    """asr_fbank_config (include/asr_amd.h)."""
    _fields_ = [("sample_rate", _f), ("win_length", _i), ("hop_length", _i), ("n_fft", _i), ("window", _i),
                ("preemph", _f), ("n_mels", _i), ("f_min", _f), ("f_max", _f), ("log_floor", _f),
                ("n_mfcc", _i), ("n_context", _i)]


class FeatureFrontend:
    """Waveform -> log-mel / MFCC features with a +-n_context frame window
    (asr_fbank_*; the semantics are in include/asr_amd.h), DeepSpeech's input
    (26 MFCCs, baseline/model.py:23) by default.  window: "hann", "hamming",
    "rect" or an ASR_FBANK_WIN_* value; f_max None = sample_rate / 2.  No
    arithmetic here: the tables and the kernels are the library's."""

    def __init__(self, sample_rate: float = 16000.0, win_length: int = 400, hop_length: int = 160,
                 n_fft: int = 512, window="hann", preemph: float = 0.97, n_mels: int = 40, f_min: float = 0.0,
                 f_max: Optional[float] = None, log_floor: float = 1e-10, n_mfcc: int = 26, n_context: int = 0):
        self.h = None
        self.cfg = FbankConfig(sample_rate, win_length, hop_length, n_fft,
                               FBANK_WINDOWS[window] if isinstance(window, str) else int(window), preemph, n_mels,
                               f_min, sample_rate / 2 if f_max is None else f_max, log_floor, n_mfcc, n_context)
        h = _vp()
        check(lib().asr_fbank_create(ctypes.byref(self.cfg), ctypes.byref(h)), "asr_fbank_create")
        self.h = h.value
        self._work: Optional[DeviceBytes] = None
        self._keep = None   # the last call's uploaded inputs: alive until its kernels are done

    def num_frames(self, n_samples: int) -> int:
        return int(lib().asr_fbank_num_frames(ctypes.byref(self.cfg), int(n_samples)))

    @property
    def feature_dim(self) -> int:
        return int(lib().asr_fbank_feature_dim(ctypes.byref(self.cfg)))

    def host_tables(self) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """(window [win_length], mel [n_mels, n_fft/2 + 1], dct [n_mfcc, n_mels] or
        None): the fp32 tables the device uses."""
        c = self.cfg
        win = np.zeros(c.win_length, np.float32)
        mel = np.zeros((c.n_mels, c.n_fft // 2 + 1), np.float32)
        dct = np.zeros((c.n_mfcc, c.n_mels), np.float32) if c.n_mfcc else None
        check(lib().asr_fbank_host_tables(ctypes.byref(c), _ptr(win), _ptr(mel), _ptr(dct) if c.n_mfcc else None),
              "asr_fbank_host_tables")
        return win, mel, dct

    def workspace_bytes(self, T: int, B: int) -> int:
        return int(lib().asr_fbank_workspace_bytes(self.h, T, B))

    def forward(self, wave, nsamples=None, stream: Optional[int] = None, B: Optional[int] = None,
                S: Optional[int] = None, ldw: Optional[int] = None, T: Optional[int] = None):
        """wave: a numpy [B, S] float32 array, or a device pointer (int) with B, S
        (and ldw, default S) given; nsamples: None, a sequence of B counts or a
        DeviceBytes of int32 [B].  Returns (features DeviceMatrix [T*B, F]
        time-major, frames DeviceBytes int32 [B]); T defaults to num_frames(S)
        (at least 1).  Asynchronous on stream; inputs uploaded here stay
        alive in this object until the next call."""
        st = stream or 0
        keep = []
        if isinstance(wave, np.ndarray):
            wave = np.ascontiguousarray(wave, dtype=np.float32)
            assert wave.ndim == 2, wave.shape
            B, S = wave.shape
            ldw = S
            dw = DeviceMatrix(B, S)
            dw.toGpu(wave, st)
            keep.append(dw)
            wptr = dw.ptr
        else:
            assert B is not None and S is not None, "a device pointer needs B and S"
            wptr, ldw = int(wave), int(S if ldw is None else ldw)
        if nsamples is not None and not isinstance(nsamples, DeviceBytes):
            nsamples = device_lengths(nsamples)
        keep.append(nsamples)
        T = max(1, self.num_frames(S)) if T is None else int(T)
        F = self.feature_dim
        out = DeviceMatrix(T * B, F)
        frames = DeviceBytes(4 * B)
        need = self.workspace_bytes(T, B)
        if need and (self._work is None or self._work.nbytes < need):
            self._work = DeviceBytes(need)
        check(lib().asr_fbank_fwd(self.h, wptr, ldw, nsamples.ptr if nsamples is not None else None, B, S,
                                  out.ptr, F, frames.ptr, self._work.ptr if need else None, T, st),
              "asr_fbank_fwd")
        self._keep = keep
        return out, frames

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().asr_fbank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_int32(d: DeviceBytes, n: int, stream: int = 0) -> np.ndarray:
    """Host copy of a device int32 [n] buffer (e.g. FeatureFrontend's frames)."""
    out = np.empty(n, np.int32)
    check(lib().asr_memcpy_d2h(_ptr(out), d.ptr, 4 * n, stream), "asr_memcpy_d2h")
    return out


# ----------------------------------------------------------------------- CTC
class CTCDecoder:
    """Handle over asr_ctc_*: decode time-major emissions [T][B][V]."""

    def __init__(self, V: int, beam_width: int, blank_id: int = 0,
                 codes: Optional[Sequence[int]] = None, max_states: int = 0, waves: int = 0):
        self.V, self.beam, self.blank = V, beam_width, blank_id
        self.codes = None if codes is None else np.ascontiguousarray(codes, dtype=np.int32)
        h = _vp()
        check(lib().asr_ctc_create(_ptr(self.codes) if self.codes is not None else None, V,
                                   beam_width, blank_id, max_states, ctypes.byref(h)),
              "asr_ctc_create")
        self.h = h.value
        if waves:
            check(lib().asr_ctc_set_waves(self.h, waves), "asr_ctc_set_waves")
        self._emis: Optional[DeviceBytes] = None
        self.T = self.B = 0
        self._last = None

    def config(self) -> Tuple[int, int, int]:
        ms, w, lds = _i(), _i(), _i()
        check(lib().asr_ctc_get_config(self.h, ctypes.byref(ms), ctypes.byref(w), ctypes.byref(lds)),
              "asr_ctc_get_config")
        return ms.value, w.value, lds.value

    def set_waves(self, waves: int) -> None:
        check(lib().asr_ctc_set_waves(self.h, waves), "asr_ctc_set_waves")

    def set_concurrency(self, n: int) -> None:
        """Scheduling hint: n decodes of this batch size run at once on the
        device (asr_ctc_set_concurrency); results are unchanged."""
        check(lib().asr_ctc_set_concurrency(self.h, int(n)), "asr_ctc_set_concurrency")

    def set_semantics(self, semantics: int) -> None:
        """SEMANTICS_CPU (default, the parity target) or SEMANTICS_CUDA
        (CTCBeamSearch.cu: exactly beam states, strip-then-merge last step)."""
        check(lib().asr_ctc_set_semantics(self.h, semantics), "asr_ctc_set_semantics")

    def set_result_stream(self, stream: int) -> None:
        """Run the best-path traceback and its copy to host memory on `stream`
        (a hipStream_t handle; 0: the decode's own stream)."""
        check(lib().asr_ctc_set_result_stream(self.h, ctypes.c_void_p(stream or None)), "asr_ctc_set_result_stream")

    def set_timesteps(self, on: bool) -> None:
        """Record each label's append frame in later decodes (beams_ts)."""
        check(lib().asr_ctc_set_timesteps(self.h, int(bool(on))), "asr_ctc_set_timesteps")

    def decode_device(self, d_emis: int, T: int, B: int, is_log: bool, stream: int = 0,
                      lengths: Optional[Sequence[int]] = None, frame_stride: Optional[int] = None,
                      utt_stride: Optional[int] = None) -> None:
        """Decode device emissions: element (t, b, v) at d_emis[t*frame_stride +
        b*utt_stride + v] (default time-major [T][B][V]); lengths[b] <= T."""
        fs = B * self.V if frame_stride is None else int(frame_stride)
        us = self.V if utt_stride is None else int(utt_stride)
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if ln is not None:
            assert ln.shape == (B,), (ln.shape, B)
        check(lib().asr_ctc_decode_ex(self.h, d_emis, T, B, fs, us,
                                      _ptr(ln) if ln is not None else None, int(bool(is_log)), stream),
              "asr_ctc_decode_ex")
        self.T, self.B = T, B
        self._last = (d_emis, fs, us, None if ln is None else ln.copy(), bool(is_log))   # for rescore()

    def decode_segment(self, d_emis: int, T: int, t0: int, t1: int, B: int, is_log: bool, stream: int = 0,
                       lengths: Optional[Sequence[int]] = None, frame_stride: Optional[int] = None,
                       utt_stride: Optional[int] = None) -> None:
        """Frames [t0, t1) of a T-frame batch (asr_ctc_decode_segment): d_emis
        addresses frame t0 (element (t, b, v) at d_emis + ((t - t0)*frame_stride
        + b*utt_stride + v) floats); segments in order from 0 to T, then
        best() / beams() as after decode_device."""
        fs = B * self.V if frame_stride is None else int(frame_stride)
        us = self.V if utt_stride is None else int(utt_stride)
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if ln is not None:
            assert ln.shape == (B,), (ln.shape, B)
        check(lib().asr_ctc_decode_segment(self.h, d_emis, T, t0, t1, B, fs, us,
                                           _ptr(ln) if ln is not None else None, int(bool(is_log)), stream),
              "asr_ctc_decode_segment")
        self.T, self.B = T, B
        self._last = None   # rescore() needs the whole utterances behind one pointer

    def decode(self, emis: np.ndarray, is_log: bool = False, stream: int = 0,
               lengths: Optional[Sequence[int]] = None, batch_major: bool = False) -> None:
        """Upload emissions (fp32 [T][B][V], or [B][T][V] with batch_major) and
        enqueue the decode; lengths[b] frames of utterance b are used."""
        emis = np.ascontiguousarray(emis, dtype=np.float32)
        if batch_major:
            B, T, V = emis.shape
            fs, us = V, T * V
        else:
            T, B, V = emis.shape
            fs, us = B * V, V
        assert V == self.V, (V, self.V)
        if self._emis is None or self._emis.nbytes < emis.nbytes:
            self._emis = DeviceBytes(emis.nbytes)
        check(lib().asr_memcpy_h2d(self._emis.ptr, _ptr(emis), emis.nbytes, stream), "asr_memcpy_h2d")
        self.decode_device(self._emis.ptr, T, B, is_log, stream, lengths, fs, us)

    def best_arrays(self, allow_overflow: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Best hypotheses as arrays: labels [B][T] int32 (row b valid up to
        lengths[b]), lengths [B], fp64 log-probs [B].  Reuses host buffers:
        copy them before the next call if they must persist."""
        B, T = self.B, self.T
        if getattr(self, "_best_bufs", None) is None or self._best_bufs[0].shape != (B, max(T, 1)):
            self._best_bufs = (np.zeros((B, max(T, 1)), np.int32), np.zeros(B, np.int32),
                               np.zeros(B, np.float64))
        lab, ln, lp = self._best_bufs
        rc = lib().asr_ctc_get_best(self.h, _ptr(lab), max(T, 1), _ptr(ln), _ptr(lp))
        if not (allow_overflow and rc == ASR_ERR_BEAM_OVERFLOW):
            check(rc, "asr_ctc_get_best")
        return lab, ln, lp

    def best(self, allow_overflow: bool = False) -> Tuple[List[List[int]], np.ndarray]:
        """Best label sequence and fp64 log-prob of every utterance."""
        lab, ln, lp = self.best_arrays(allow_overflow)
        return [lab[b, :ln[b]].tolist() for b in range(self.B)], lp.copy()

    def beams(self, max_hyps: int) -> List[List[Tuple[List[int], float]]]:
        """Ranked final beam (logp desc, string asc) of every utterance."""
        B, T = self.B, self.T
        nh = np.zeros(B, np.int32)
        ln = np.zeros((B, max_hyps), np.int32)
        lab = np.zeros((B, max_hyps, max(T, 1)), np.int32)
        lp = np.zeros((B, max_hyps), np.float64)
        check(lib().asr_ctc_get_beams(self.h, max_hyps, max(T, 1), _ptr(nh), _ptr(ln), _ptr(lab),
                                      _ptr(lp)), "asr_ctc_get_beams")
        return [[(lab[b, k, :ln[b, k]].tolist(), float(lp[b, k])) for k in range(min(nh[b], max_hyps))]
                for b in range(B)]

    def beams_ts(self, max_hyps: int) -> List[List[Tuple[List[int], float, List[int]]]]:
        """Ranked final beam with each label's append frame: [(labels, logp,
        timesteps)] per utterance (timesteps mode must have been on)."""
        B, T = self.B, self.T
        nh = np.zeros(B, np.int32)
        ln = np.zeros((B, max_hyps), np.int32)
        lab = np.zeros((B, max_hyps, max(T, 1)), np.int32)
        lp = np.zeros((B, max_hyps), np.float64)
        ts = np.zeros((B, max_hyps, max(T, 1)), np.int32)
        check(lib().asr_ctc_get_beams_ts(self.h, max_hyps, max(T, 1), _ptr(nh), _ptr(ln), _ptr(lab),
                                         _ptr(lp), _ptr(ts)), "asr_ctc_get_beams_ts")
        return [[(lab[b, k, :ln[b, k]].tolist(), float(lp[b, k]), ts[b, k, :ln[b, k]].tolist())
                 for k in range(min(nh[b], max_hyps))] for b in range(B)]

    def rescore(self, max_hyps: int, stream: int = 0) -> List[List[Tuple[List[int], float, float]]]:
        """The final beam re-ranked by exact CTC log-likelihood: per utterance
        [(labels, exact score, beam score)], exact score descending (equal
        scores keep their beam order).  A beam score sums only the alignments
        that survived pruning, a lower bound; the exact one is asr_ctc_align's
        forward score of every hypothesis against its utterance, one call for
        the whole batch.  After decode() / decode_device() of whole utterances
        (the emissions must still be in place)."""
        if self._last is None:
            raise AsrError(ASR_ERR_STATE, "CTCDecoder.rescore: no whole-utterance decode yet")
        d_emis, fs, us, ln, is_log = self._last
        hyps = self.beams(max_hyps)
        targets = [lab for u in hyps for lab, _ in u]
        utt = [b for b, u in enumerate(hyps) for _ in u]
        if not targets:
            return [[] for _ in hyps]
        exact = ctc_score(d_emis, targets, lengths=ln, utt=utt, is_log=is_log, blank=self.blank,
                          shape=(self.T, self.B, self.V), frame_stride=fs, utt_stride=us, stream=stream)
        out, k = [], 0
        for u in hyps:
            rows = [(lab, float(exact[k + j]), lp) for j, (lab, lp) in enumerate(u)]
            k += len(u)
            out.append(sorted(rows, key=lambda r: -r[1]))
        return out

    def lm_rescore(self, max_hyps: int, lm: "NGramLM", alpha: float, beta: float, mapper, bos: bool = True,
                   eos: bool = True, stream: int = 0) -> List[List[Tuple[List[int], float, float, float, int]]]:
        """The final beam re-ranked with a language model: per utterance
        [(labels, total, exact_ctc, lm_log10, n_tokens)], total descending (equal
        totals keep their beam order), with ctcdecode's combination
            total = exact_ctc + alpha * ln(10) * lm_log10 + beta * n_tokens.
        exact_ctc is rescore()'s exact score (natural log); mapper turns a label
        list into LM token ids (NGramLM.label_mapper); lm_log10 is the LM's
        log10 probability of those tokens (one asr_lm_score launch for the whole
        batch; lm.upload() first) and n_tokens the tokens scored without </s>.
        After decode() / decode_device() of whole utterances, as rescore()."""
        if self._last is None:
            raise AsrError(ASR_ERR_STATE, "CTCDecoder.lm_rescore: no whole-utterance decode yet")
        d_emis, fs, us, ln, is_log = self._last
        hyps = self.beams(max_hyps)
        targets = [lab for u in hyps for lab, _ in u]
        utt = [b for b, u in enumerate(hyps) for _ in u]
        if not targets:
            return [[] for _ in hyps]
        exact = ctc_score(d_emis, targets, lengths=ln, utt=utt, is_log=is_log, blank=self.blank,
                          shape=(self.T, self.B, self.V), frame_stride=fs, utt_stride=us, stream=stream)
        lm_log10, counts = lm.score([mapper(lab) for lab in targets], bos=bos, eos=eos, stream=stream)
        n_tok = np.asarray(counts)[:, 0] - (1 if eos else 0)
        out, k = [], 0
        for u in hyps:
            rows = [(lab, lm_total(float(exact[k + j]), float(lm_log10[k + j]), int(n_tok[k + j]), alpha, beta),
                     float(exact[k + j]), float(lm_log10[k + j]), int(n_tok[k + j])) for j, (lab, _) in enumerate(u)]
            k += len(u)
            out.append(sorted(rows, key=lambda r: -r[1]))
        return out

    def attention_rescore(self, max_hyps: int, decoder: "TransformerDecoder", memory, T: int, enc_lengths=None,
                          ctc_weight: float = 0.5, sos: Optional[int] = None, eos: Optional[int] = None,
                          stream: int = 0) -> List[List[Tuple[List[int], float, float, float]]]:
        """The final beam re-ranked by an attention decoder: per utterance
        [(labels, total, att, exact_ctc)], total = att + ctc_weight * exact_ctc
        descending (equal totals keep their beam order).  exact_ctc is
        rescore()'s exact score (ctc_score, one call for the batch); att is
        decoder.score() of the hypothesis teacher-forced against the encoder
        output memory [T*B, E] (device, T its frames, enc_lengths its frames
        per utterance) — one grouped cross-attention launch per decoder layer
        for the whole batch, the memory projected once per utterance.  After
        decode() / decode_device() of whole utterances, as rescore()."""
        if self._last is None:
            raise AsrError(ASR_ERR_STATE, "CTCDecoder.attention_rescore: no whole-utterance decode yet")
        d_emis, fs, us, ln, is_log = self._last
        hyps = self.beams(max_hyps)
        targets = [lab for u in hyps for lab, _ in u]
        utt = [b for b, u in enumerate(hyps) for _ in u]
        if not targets:
            return [[] for _ in hyps]
        exact = ctc_score(d_emis, targets, lengths=ln, utt=utt, is_log=is_log, blank=self.blank,
                          shape=(self.T, self.B, self.V), frame_stride=fs, utt_stride=us, stream=stream)
        att = decoder.score(targets, utt, memory, T, self.B, enc_lengths, sos, eos, stream)
        return attention_combine(hyps, att, exact, ctc_weight)

    def mbr_rescore(self, max_hyps: int, scale: float = 1.0, lm: Optional["NGramLM"] = None, alpha: float = 0.0,
                    beta: float = 0.0, mapper=None, tokens=None,
                    stream: int = 0) -> List[List[Tuple[List[int], float, float]]]:
        """The final beam re-ranked by minimum Bayes risk: per utterance [(labels,
        risk, total)], risk ascending (equal risks keep the order of the ranking
        they came from).  risk is the expected edit distance to the other
        hypotheses of the beam under the weights scale * total (natural log),
        where total is rescore()'s exact CTC score or, with lm, lm_rescore()'s
        total (alpha, beta and mapper as there).  Distances are taken over the
        labels, or over tokens(labels) when tokens is given (word_tokens for word
        error).  One asr_nbest_mbr call for the whole batch (max_hyps <=
        ASR_MBR_MAX_HYPS).  After decode() / decode_device() of whole utterances,
        as rescore()."""
        if self._last is None:
            raise AsrError(ASR_ERR_STATE, "CTCDecoder.mbr_rescore: no whole-utterance decode yet")
        if lm is not None:
            ranked = [[(r[0], r[1]) for r in u] for u in self.lm_rescore(max_hyps, lm, alpha, beta, mapper,
                                                                         stream=stream)]
        else:
            ranked = [[(r[0], r[1]) for r in u] for u in self.rescore(max_hyps, stream=stream)]
        seqs = [[list(tokens(lab)) if tokens is not None else lab for lab, _ in u] for u in ranked]
        weights = [[scale * total for _, total in u] for u in ranked]
        risks, _, _ = nbest_mbr(seqs, weights, stream=stream)
        return [sorted(((lab, float(risks[b][j]), total) for j, (lab, total) in enumerate(u)), key=lambda r: r[1])
                for b, u in enumerate(ranked)]

    def last_kernel_ms(self) -> float:
        ms = _f()
        check(lib().asr_ctc_last_kernel_ms(self.h, ctypes.byref(ms)), "asr_ctc_last_kernel_ms")
        return ms.value

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().asr_ctc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------- CTC alignment and scoring
def ctc_align_workspace_bytes(T: int, N: int, max_target_len: int) -> int:
    """Bytes of d_work for asr_ctc_align with a path or spans wanted (0: invalid shape)."""
    return int(lib().asr_ctc_align_workspace_bytes(T, N, max_target_len))


def ctc_align_device(d_emis: int, T: int, B: int, V: int, frame_stride: int, utt_stride: int, d_lengths: int,
                     is_log: bool, blank: int, d_targets: int, ldt: int, d_target_lengths: int, d_utt: int,
                     N: int, max_target_len: int, d_score: int = 0, d_vscore: int = 0, d_path: int = 0,
                     ldp: int = 0, d_spans: int = 0, d_work: int = 0, stream: int = 0) -> None:
    """asr_ctc_align over raw device pointers (0 = NULL); asynchronous on stream."""
    check(lib().asr_ctc_align(d_emis, T, B, V, frame_stride, utt_stride, d_lengths or None, int(bool(is_log)),
                              blank, d_targets, ldt, d_target_lengths, d_utt or None, N, max_target_len,
                              d_score or None, d_vscore or None, d_path or None, ldp, d_spans or None,
                              d_work or None, stream or None), "asr_ctc_align")


def _upload(a: np.ndarray, stream: int = 0) -> DeviceBytes:
    a = np.ascontiguousarray(a)
    d = DeviceBytes(max(a.nbytes, 16))
    check(lib().asr_memcpy_h2d(d.ptr, _ptr(a), a.nbytes, stream), "asr_memcpy_h2d")
    return d


def _download(d: DeviceBytes, shape, dtype, stream: int = 0) -> np.ndarray:
    out = np.empty(shape, dtype)
    check(lib().asr_memcpy_d2h(_ptr(out), d.ptr, out.nbytes, stream), "asr_memcpy_d2h")
    return out


def _ctc_align_call(emis, targets, lengths, utt, is_log, blank, batch_major, shape, frame_stride, utt_stride,
                    stream, want_score, want_vscore, want_path):
    """Shared body of ctc_score / ctc_align: upload, one asr_ctc_align, download."""
    keep = []
    if isinstance(emis, (int, np.integer)):
        if shape is None:
            raise ValueError("a device pointer needs shape=(T, B, V)")
        T, B, V = (int(x) for x in shape)
        d_emis = int(emis)
        fs = (V if batch_major else B * V) if frame_stride is None else int(frame_stride)
        us = (T * V if batch_major else V) if utt_stride is None else int(utt_stride)
    else:
        emis = np.ascontiguousarray(emis, dtype=np.float32)
        if batch_major:
            B, T, V = emis.shape
            fs, us = V, T * V
        else:
            T, B, V = emis.shape
            fs, us = B * V, V
        keep.append(_upload(emis, stream))
        d_emis = keep[-1].ptr
    N = len(targets)
    mtl = max([len(t) for t in targets] + [0])
    ldt = max(mtl, 1)
    tg = np.zeros((N, ldt), np.int32)
    for n, t in enumerate(targets):
        tg[n, :len(t)] = np.asarray(t, dtype=np.int32)
    tl = np.array([len(t) for t in targets], np.int32)
    d_tg, d_tl = _upload(tg, stream), _upload(tl, stream)
    d_len = d_utt = None
    if lengths is not None:
        ln = np.ascontiguousarray(lengths, dtype=np.int32)
        assert ln.shape == (B,), (ln.shape, B)
        d_len = _upload(ln, stream)
    if utt is not None:
        ut = np.ascontiguousarray(utt, dtype=np.int32)
        assert ut.shape == (N,), (ut.shape, N)
        d_utt = _upload(ut, stream)
    d_score = DeviceBytes(8 * N) if want_score else None
    d_vscore = DeviceBytes(8 * N) if want_vscore else None
    d_path = d_spans = d_work = None
    if want_path:
        d_path = DeviceBytes(4 * N * T)
        d_spans = DeviceBytes(8 * N * ldt)
        d_work = DeviceBytes(max(ctc_align_workspace_bytes(T, N, mtl), 16))
    ctc_align_device(d_emis, T, B, V, fs, us, d_len.ptr if d_len else 0, is_log, blank, d_tg.ptr, ldt, d_tl.ptr,
                     d_utt.ptr if d_utt else 0, N, mtl, d_score.ptr if d_score else 0,
                     d_vscore.ptr if d_vscore else 0, d_path.ptr if d_path else 0, T,
                     d_spans.ptr if d_spans else 0, d_work.ptr if d_work else 0, stream)
    score = _download(d_score, N, np.float64, stream) if want_score else None
    vscore = _download(d_vscore, N, np.float64, stream) if want_vscore else None
    paths = spans = None
    if want_path:
        pa = _download(d_path, (N, T), np.int32, stream)
        sp = _download(d_spans, (N, ldt, 2), np.int32, stream)
        # frames past the utterance's length are -1; so is every frame of an infeasible target
        paths =[pa[n, :int((pa[n] >= 0).sum())].copy() for n in range(N)]
        spans = [sp[n, :len(targets[n])].copy() for n in range(N)]
    return score, vscore, paths, spans


def ctc_score(emis, targets: Sequence[Sequence[int]], lengths: Optional[Sequence[int]] = None,
              utt: Optional[Sequence[int]] = None, is_log: bool = False, blank: int = 0,
              batch_major: bool = False, shape: Optional[Tuple[int, int, int]] = None,
              frame_stride: Optional[int] = None, utt_stride: Optional[int] = None, stream: int = 0) -> np.ndarray:
    """Exact CTC forward log-likelihood log p(target | emissions) of every
    target, fp64 [N] (-inf: infeasible).  emis: numpy [T][B][V] ([B][T][V] with
    batch_major), or a device pointer with shape=(T, B, V).  targets: a list of
    label lists; target n is scored against utterance utt[n] (default n).
    lengths[b]: frames of utterance b (default T)."""
    return _ctc_align_call(emis, targets, lengths, utt, is_log, blank, batch_major, shape, frame_stride,
                           utt_stride, stream, True, False, False)[0]


def ctc_align(emis, targets: Sequence[Sequence[int]], lengths: Optional[Sequence[int]] = None,
              utt: Optional[Sequence[int]] = None, is_log: bool = False, blank: int = 0,
              batch_major: bool = False, shape: Optional[Tuple[int, int, int]] = None,
              frame_stride: Optional[int] = None, utt_stride: Optional[int] = None,
              stream: int = 0) -> Tuple[np.ndarray, List[np.ndarray], List[np.ndarray]]:
    """Viterbi forced alignment (torchaudio.functional.forced_align semantics):
    (vscore fp64 [N], paths, spans).  paths[n]: the label emitted at each of the
    utterance's frames, blank included (empty when the target is infeasible);
    spans[n]: int32 [L_n, 2], first frame and one past the last frame of each
    target label ((-1, -1) when infeasible).  Arguments as ctc_score."""
    _, vscore, paths, spans = _ctc_align_call(emis, targets, lengths, utt, is_log, blank, batch_major, shape,
                                              frame_stride, utt_stride, stream, False, True, True)
    return vscore, paths, spans


# ------------------------------------------------------- n-gram language model
ASR_LM_MAX_ORDER = 8
ASR_LM_BOS, ASR_LM_EOS = 1, 2
LN10 = math.log(10.0)


class LmInfo(ctypes.Structure):
    """asr_lm_info (include/asr_amd.h)."""
    _fields_ = [("order", ctypes.c_int32), ("vocab", ctypes.c_int32), ("bos_id", ctypes.c_int32),
                ("eos_id", ctypes.c_int32), ("unk_id", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("ngrams", ctypes.c_int64 * ASR_LM_MAX_ORDER), ("nodes_inserted", ctypes.c_int64),
                ("table_bytes", ctypes.c_int64)]


def lm_total(exact_ctc: float, lm_log10: float, n_tokens: int, alpha: float, beta: float) -> float:
    """ctcdecode's combination of an acoustic score (natural log), an LM score
    (log10) and a word bonus."""
    return exact_ctc + alpha * LN10 * lm_log10 + beta * n_tokens


class NGramLM:
    """Back-off n-gram language model (asr_lm_*; the semantics are in
    include/asr_amd.h): an ARPA file parsed into an exact table on the host,
    scored on the host (host=True) or, after upload(), on the device, one wave
    per hypothesis.  No arithmetic here."""

    def __init__(self, handle: int):
        self.h = handle
        info = LmInfo()
        check(lib().asr_lm_get_info(self.h, ctypes.byref(info)), "asr_lm_get_info")
        self.order, self.vocab_size = int(info.order), int(info.vocab)
        self.bos_id, self.eos_id, self.unk_id = int(info.bos_id), int(info.eos_id), int(info.unk_id)

    @classmethod
    def from_arpa(cls, path, oov_log10: float = -100.0) -> "NGramLM":
        h = _vp()
        check(lib().asr_lm_create_arpa(os.fsencode(path), oov_log10, ctypes.byref(h)), "asr_lm_create_arpa")
        return cls(h.value)

    @classmethod
    def from_string(cls, text, oov_log10: float = -100.0) -> "NGramLM":
        data = text.encode() if isinstance(text, str) else bytes(text)
        h = _vp()
        check(lib().asr_lm_create_arpa_mem(data, len(data), oov_log10, ctypes.byref(h)), "asr_lm_create_arpa_mem")
        return cls(h.value)

    def info(self) -> dict:
        info = LmInfo()
        check(lib().asr_lm_get_info(self.h, ctypes.byref(info)), "asr_lm_get_info")
        return {"order": int(info.order), "vocab": int(info.vocab), "bos_id": int(info.bos_id),
                "eos_id": int(info.eos_id), "unk_id": int(info.unk_id),
                "ngrams": [int(info.ngrams[k]) for k in range(int(info.order))],
                "nodes_inserted": int(info.nodes_inserted), "table_bytes": int(info.table_bytes)}

    def token_id(self, token: str) -> int:
        """The token's id, -1 when the model does not have it."""
        i = ctypes.c_int32(-1)
        check(lib().asr_lm_token_id(self.h, token.encode(), ctypes.byref(i)), "asr_lm_token_id")
        return int(i.value)

    def token_string(self, token_id: int) -> str:
        s = ctypes.c_char_p()
        check(lib().asr_lm_token_string(self.h, int(token_id), ctypes.byref(s)), "asr_lm_token_string")
        return s.value.decode()

    def upload(self) -> None:
        """Copy the tables to the current device (synchronous; once)."""
        check(lib().asr_lm_upload(self.h), "asr_lm_upload")

    def score(self, token_lists: Sequence[Sequence[int]], bos: bool = True, eos: bool = True, detail: bool = False,
              host: bool = False, stream: int = 0):
        """(log10 probability [N] float64, counts [N, 2] int32: tokens scored with
        </s>, OOVs); with detail also the per-token log10 values and matched
        orders as lists of arrays (the </s> entry last).  host=True runs
        asr_lm_score_host; otherwise one asr_lm_score launch on stream."""
        N = len(token_lists)
        flags = (ASR_LM_BOS if bos else 0) | (ASR_LM_EOS if eos else 0)
        if N == 0:
            empty = (np.zeros(0, np.float64), np.zeros((0, 2), np.int32))
            return empty + ([], []) if detail else empty
        max_len = max(len(t) for t in token_lists)
        ldt, ldd = max(max_len, 1), max_len + 1
        tok = np.zeros((N, ldt), np.int32)
        for n, t in enumerate(token_lists):
            tok[n, :len(t)] = np.asarray(t, dtype=np.int32)
        ln = np.array([len(t) for t in token_lists], np.int32)
        if host:
            logp, counts = np.zeros(N, np.float64), np.zeros((N, 2), np.int32)
            tl = np.zeros((N, ldd), np.float64) if detail else None
            to = np.zeros((N, ldd), np.int32) if detail else None
            check(lib().asr_lm_score_host(self.h, _ptr(tok), ldt, _ptr(ln), N, max_len, flags, _ptr(logp),
                                          _ptr(counts), _ptr(tl) if detail else None,
                                          _ptr(to) if detail else None, ldd), "asr_lm_score_host")
        else:
            d_tok, d_ln = _upload(tok, stream), _upload(ln, stream)
            d_logp, d_counts = DeviceBytes(8 * N), DeviceBytes(8 * N)
            d_tl = DeviceBytes(8 * N * ldd) if detail else None
            d_to = DeviceBytes(4 * N * ldd) if detail else None
            check(lib().asr_lm_score(self.h, d_tok.ptr, ldt, d_ln.ptr, N, max_len, flags, d_logp.ptr, d_counts.ptr,
                                     d_tl.ptr if detail else None, d_to.ptr if detail else None, ldd,
                                     stream or None), "asr_lm_score")
            logp = _download(d_logp, N, np.float64, stream)
            counts = _download(d_counts, (N, 2), np.int32, stream)
            tl = _download(d_tl, (N, ldd), np.float64, stream) if detail else None
            to = _download(d_to, (N, ldd), np.int32, stream) if detail else None
        if not detail:
            return logp, counts
        return (logp, counts, [tl[n, :counts[n, 0]].copy() for n in range(N)],
                [to[n, :counts[n, 0]].copy() for n in range(N)])

    def label_mapper(self, labels: Sequence[str], mode: str = "char", space: str = " "):
        """A function from a hypothesis (label ids) to this model's token ids, on
        the host.  labels[i] is label i's string.  "char": every label's string
        is looked up as a token, labels with an empty string (the blank) are
        dropped; "word": the label strings are joined, split at `space`, and
        every non-empty word is looked up.  An unknown token maps to -1 (OOV)."""
        if mode not in ("char", "word"):
            raise ValueError(f"label_mapper: mode {mode!r}")
        labels = list(labels)
        cache: dict = {}

        def lookup(s: str) -> int:
            if s not in cache:
                cache[s] = self.token_id(s)
            return cache[s]

        if mode == "char":
            def mapper(hyp):
                return [lookup(labels[c]) for c in hyp if labels[c] != ""]
        else:
            def mapper(hyp):
                return [lookup(w) for w in "".join(labels[c] for c in hyp).split(space) if w != ""]
        return mapper

    def label_tokens(self, labels: Sequence[str]) -> np.ndarray:
        """int32 [V]: every label's string looked up as a token of this model
        (CTCLMDecoder's tok_of_label); the empty string or an absent token
        gives -1 (an OOV)."""
        return np.array([self.token_id(s) if s != "" else -1 for s in labels], dtype=np.int32)

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().asr_lm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ASR_LEX_OPEN, ASR_LEX_CLOSED = 0, 1


class LexiconInfo(ctypes.Structure):
    """asr_lexicon_info (include/asr_amd.h)."""
    _fields_ = [("words", ctypes.c_int32), ("nodes", ctypes.c_int32), ("max_children", ctypes.c_int32),
                ("space_label", ctypes.c_int32), ("table_bytes", ctypes.c_int64)]


class Lexicon:
    """Handle over asr_lexicon_*: words spelled in label ids, each with one LM
    token id, as a trie (include/asr_amd.h).  words is a list of label-id
    lists, tokens their LM token ids, V the number of labels and space the
    space label's id.  No arithmetic here."""

    def __init__(self, words: Sequence[Sequence[int]], tokens: Sequence[int], V: int, space: int):
        words = [list(w) for w in words]
        if len(words) != len(tokens):
            raise ValueError(f"Lexicon: {len(words)} words, {len(tokens)} tokens")
        spell = np.ascontiguousarray([c for w in words for c in w] or [0], dtype=np.int32)
        offsets = np.zeros(len(words) + 1, np.int64)
        offsets[1:] = np.cumsum([len(w) for w in words])
        tok = np.ascontiguousarray(list(tokens) or [0], dtype=np.int32)
        h = _vp()
        check(lib().asr_lexicon_create(_ptr(spell), _ptr(offsets), _ptr(tok), len(words), V, space, ctypes.byref(h)),
              "asr_lexicon_create")
        self.h = h.value
        self.V, self.space, self.skipped = V, space, 0

    @classmethod
    def from_lm(cls, lm: "NGramLM", labels: Sequence[str], space: str = " ",
                blank_id: Optional[int] = None) -> "Lexicon":
        """Every token of lm except <s>, </s> and <unk>, spelled character by
        character in labels.  A token with a character that is no label, or
        with the space, is left out; `skipped` counts those.  blank_id names a
        label whose string (ctcdecode's "_") spells nothing."""
        labels = list(labels)
        if space not in labels:
            raise ValueError(f"Lexicon.from_lm: the space {space!r} is not a label")
        label_of = {s: i for i, s in enumerate(labels) if len(s) == 1 and i != blank_id}
        words, tokens, skipped = [], [], 0
        for t in range(lm.vocab_size):
            if t in (lm.bos_id, lm.eos_id, lm.unk_id):
                continue
            s = lm.token_string(t)
            if s == "" or space in s or any(ch not in label_of for ch in s):
                skipped += 1
                continue
            words.append([label_of[ch] for ch in s])
            tokens.append(t)
        lex = cls(words, tokens, len(labels), labels.index(space))
        lex.skipped = skipped
        return lex

    def upload(self) -> None:
        """Copy the trie to the current device (synchronous; once)."""
        check(lib().asr_lexicon_upload(self.h), "asr_lexicon_upload")

    def info(self) -> dict:
        info = LexiconInfo()
        check(lib().asr_lexicon_get_info(self.h, ctypes.byref(info)), "asr_lexicon_get_info")
        return {"words": int(info.words), "nodes": int(info.nodes), "max_children": int(info.max_children),
                "space_label": int(info.space_label), "table_bytes": int(info.table_bytes)}

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().asr_lexicon_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CTCLMDecoder:
    """Handle over asr_ctc_lm_*: the beam search with the n-gram LM fused into
    every prune (the semantics are in include/asr_amd.h).  lm is an NGramLM
    that must outlive this decoder (upload() it before a device decode);
    tok_of_label[V] is the LM token of every label (NGramLM.label_tokens).
    CTCLMDecoder.word(...) is the same handle in the word mode: a word-level
    LM fused through a Lexicon.  No arithmetic here."""

    def __init__(self, V: int, beam_width: int, lm: NGramLM, tok_of_label: Sequence[int], alpha: float, beta: float,
                 blank_id: int = 0, bos: bool = True, eos: bool = False, top_n: int = 0, max_states: int = 0,
                 codes: Optional[Sequence[int]] = None):
        self.V, self.beam, self.blank = V, beam_width, blank_id
        self.lm = lm   # keeps the LM handle alive
        self.codes = None if codes is None else np.ascontiguousarray(codes, dtype=np.int32)
        tok = np.ascontiguousarray(tok_of_label, dtype=np.int32)
        if tok.shape != (V,):
            raise ValueError(f"CTCLMDecoder: tok_of_label has shape {tok.shape}, not ({V},)")
        flags = (ASR_LM_BOS if bos else 0) | (ASR_LM_EOS if eos else 0)
        h = _vp()
        check(lib().asr_ctc_lm_create(_ptr(self.codes) if self.codes is not None else None, V, beam_width, blank_id,
                                      max_states, lm.h, _ptr(tok), alpha, beta, flags, top_n, ctypes.byref(h)),
              "asr_ctc_lm_create")
        self.h = h.value
        self.lexicon: Optional[Lexicon] = None
        self._emis: Optional[DeviceBytes] = None
        self.T = self.B = 0

    @classmethod
    def word(cls, V: int, beam_width: int, lm: NGramLM, lexicon: Lexicon, alpha: float, beta: float,
             blank_id: int = 0, bos: bool = True, eos: bool = False, top_n: int = 0, closed: bool = False,
             max_states: int = 0, codes: Optional[Sequence[int]] = None) -> "CTCLMDecoder":
        """The word mode (asr_ctc_lm_create_word): lm is a word-level model and
        lexicon spells its words; closed=True keeps the search inside the
        lexicon.  beams() then reports words as n_tokens.  lm and lexicon must
        outlive the decoder (upload() both before a device decode)."""
        self = cls.__new__(cls)
        self.V, self.beam, self.blank = V, beam_width, blank_id
        self.lm, self.lexicon = lm, lexicon   # keeps both handles alive
        self.codes = None if codes is None else np.ascontiguousarray(codes, dtype=np.int32)
        flags = (ASR_LM_BOS if bos else 0) | (ASR_LM_EOS if eos else 0)
        h = _vp()
        self.h = None
        check(lib().asr_ctc_lm_create_word(_ptr(self.codes) if self.codes is not None else None, V, beam_width,
                                           blank_id, max_states, lm.h, lexicon.h, alpha, beta, flags, top_n,
                                           ASR_LEX_CLOSED if closed else ASR_LEX_OPEN, ctypes.byref(h)),
              "asr_ctc_lm_create_word")
        self.h = h.value
        self._emis = None
        self.T = self.B = 0
        return self

    @staticmethod
    def _lengths(lengths, B):
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if ln is not None:
            assert ln.shape == (B,), (ln.shape, B)
        return ln

    def decode_device(self, d_emis: int, T: int, B: int, is_log: bool, stream: int = 0,
                      lengths: Optional[Sequence[int]] = None, frame_stride: Optional[int] = None,
                      utt_stride: Optional[int] = None) -> None:
        """Decode device emissions: element (t, b, v) at d_emis[t*frame_stride +
        b*utt_stride + v] (default time-major [T][B][V]); 1 <= lengths[b] <= T."""
        fs = B * self.V if frame_stride is None else int(frame_stride)
        us = self.V if utt_stride is None else int(utt_stride)
        ln = self._lengths(lengths, B)
        check(lib().asr_ctc_lm_decode(self.h, d_emis, T, B, fs, us, _ptr(ln) if ln is not None else None,
                                      int(bool(is_log)), stream or None), "asr_ctc_lm_decode")
        self.T, self.B = T, B

    @staticmethod
    def _shape(emis, batch_major):
        if batch_major:
            B, T, V = emis.shape
            return T, B, V, V, T * V
        T, B, V = emis.shape
        return T, B, V, B * V, V

    def decode(self, emis: np.ndarray, is_log: bool = False, stream: int = 0,
               lengths: Optional[Sequence[int]] = None, batch_major: bool = False) -> None:
        """Upload emissions (fp32 [T][B][V], or [B][T][V] with batch_major) and
        enqueue the decode on the device."""
        emis = np.ascontiguousarray(emis, dtype=np.float32)
        T, B, V, fs, us = self._shape(emis, batch_major)
        assert V == self.V, (V, self.V)
        if self._emis is None or self._emis.nbytes < emis.nbytes:
            self._emis = DeviceBytes(emis.nbytes)
        check(lib().asr_memcpy_h2d(self._emis.ptr, _ptr(emis), emis.nbytes, stream), "asr_memcpy_h2d")
        self.decode_device(self._emis.ptr, T, B, is_log, stream, lengths, fs, us)

    def decode_host(self, emis: np.ndarray, is_log: bool = False, lengths: Optional[Sequence[int]] = None,
                    batch_major: bool = False) -> None:
        """The host twin (asr_ctc_lm_decode_host): one thread, no GPU."""
        emis = np.ascontiguousarray(emis, dtype=np.float32)
        T, B, V, fs, us = self._shape(emis, batch_major)
        assert V == self.V, (V, self.V)
        ln = self._lengths(lengths, B)
        check(lib().asr_ctc_lm_decode_host(self.h, _ptr(emis), T, B, fs, us, _ptr(ln) if ln is not None else None,
                                           int(bool(is_log))), "asr_ctc_lm_decode_host")
        self.T, self.B = T, B

    def beams(self, max_hyps: int) -> List[List[Tuple[List[int], float, float, float, int]]]:
        """Ranked final beam (total desc, string asc) of every utterance of the
        last decode: [(labels, total, ctc_logp, lm_log10, n_tokens)]."""
        B, T = self.B, max(self.T, 1)
        nh = np.zeros(max(B, 1), np.int32)
        ln = np.zeros((B, max_hyps), np.int32)
        lab = np.zeros((B, max_hyps, T), np.int32)
        tot, ctc, lm = (np.zeros((B, max_hyps), np.float64) for _ in range(3))
        nt = np.zeros((B, max_hyps), np.int32)
        check(lib().asr_ctc_lm_get_beams(self.h, max_hyps, T, _ptr(nh), _ptr(ln), _ptr(lab), _ptr(tot), _ptr(ctc),
                                         _ptr(lm), _ptr(nt)), "asr_ctc_lm_get_beams")
        return [[(lab[b, k, :ln[b, k]].tolist(), float(tot[b, k]), float(ctc[b, k]), float(lm[b, k]), int(nt[b, k]))
                 for k in range(min(nh[b], max_hyps))] for b in range(B)]

    def host_gaps(self) -> np.ndarray:
        """Per utterance of the last decode_host: the smallest relative gap
        between two differing scores whose order decided something
        (asr_ctc_lm_host_gaps)."""
        g = np.zeros(max(self.B, 1), np.float64)
        check(lib().asr_ctc_lm_host_gaps(self.h, _ptr(g)), "asr_ctc_lm_host_gaps")
        return g[:self.B].copy()

    def best(self) -> Tuple[List[List[int]], np.ndarray]:
        """Best label sequence and total of every utterance."""
        B, T = self.B, max(self.T, 1)
        lab = np.zeros((max(B, 1), T), np.int32)
        ln = np.zeros(max(B, 1), np.int32)
        tot = np.zeros(max(B, 1), np.float64)
        check(lib().asr_ctc_lm_get_best(self.h, _ptr(lab), T, _ptr(ln), _ptr(tot)), "asr_ctc_lm_get_best")
        return [lab[b, :ln[b]].tolist() for b in range(B)], tot[:B].copy()

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().asr_ctc_lm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------ RNN-T (transducer)
RNNT_ACT_RELU, RNNT_ACT_TANH = 0, 1    # ASR_RNNT_ACT_*
RNNT_ACTS = {"relu": RNNT_ACT_RELU, "tanh": RNNT_ACT_TANH}
RNNT_LATTICE_STANDARD, RNNT_LATTICE_ONE_PER_FRAME = 0, 1   # asr_rnnt_align's topology
RNNT_TOPOLOGIES = {"standard": RNNT_LATTICE_STANDARD, "one_per_frame": RNNT_LATTICE_ONE_PER_FRAME}
ASR_RNNT_MAX_LAYERS = 2


class RnntDesc(ctypes.Structure):
    """asr_rnnt_desc (include/asr_amd.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("V", "blank", "E", "D", "Hp", "L", "J", "act", "max_symbols")]


class RnntWeights(ctypes.Structure):
    """asr_rnnt_weights: host pointers."""
    _fields_ = [("emb", _vp), ("w_ih", _vp * ASR_RNNT_MAX_LAYERS), ("w_hh", _vp * ASR_RNNT_MAX_LAYERS),
                ("b_ih", _vp * ASR_RNNT_MAX_LAYERS), ("b_hh", _vp * ASR_RNNT_MAX_LAYERS), ("w_enc", _vp),
                ("b_enc", _vp), ("w_pred", _vp), ("b_pred", _vp), ("w_out", _vp), ("b_out", _vp)]


class RnntInfo(ctypes.Structure):
    """asr_rnnt_info."""
    _fields_ = [("desc", RnntDesc), ("uploaded", ctypes.c_int32), ("lds_bytes", ctypes.c_int32),
                ("weight_bytes", ctypes.c_int64)]


def rnnt_desc(V: int, blank: int, E: int, D: int, Hp: int, L: int, J: int, act="relu",
              max_symbols: int = 10) -> RnntDesc:
    return RnntDesc(V, blank, E, D, Hp, L, J, RNNT_ACTS[act] if isinstance(act, str) else int(act), max_symbols)


class TransducerDecoder:
    """RNN-T greedy decoding (asr_rnnt_*; the walk is defined in
    include/asr_amd.h): an embedding, an LSTM prediction network of one or two
    layers and a joint network, decoded frame by frame in one launch
    (decode / decode_device) or by the fp64 host twin (decode_host); and the
    one-symbol-per-frame beam search on the same handle (beam_search /
    beam_search_device / beam_search_host), with an NGramLM optionally fused
    into every prune (the lm keywords; asr_rnnt_lm_*).  No arithmetic here.

    weights: a dict of fp32 arrays in the library's [in][out] layout: emb
    [V, D]; w_ih, w_hh, b_ih, b_hh: lists of L arrays ([in, 4Hp], [Hp, 4Hp],
    [4Hp]); w_enc [E, J], b_enc; w_pred [Hp, J], b_pred; w_out [J, V], b_out.
    labels (optional): label i's string, by which the LM keywords find the LM
    token of a label when no tok_of_label is given."""

    def __init__(self, desc: RnntDesc, weights: dict, labels: Optional[Sequence[str]] = None):
        self.desc = desc
        self.h = None
        self.labels = list(labels) if labels is not None else None
        self._fuse = {}
        d = desc
        L = max(0, min(int(d.L), ASR_RNNT_MAX_LAYERS))
        H4 = 4 * d.Hp
        shapes = {"emb": (d.V, d.D), "w_enc": (d.E, d.J), "b_enc": (d.J,), "w_pred": (d.Hp, d.J), "b_pred": (d.J,),
                  "w_out": (d.J, d.V), "b_out": (d.V,)}
        keep = {}
        w = RnntWeights()
        for name, shape in shapes.items():
            a = np.ascontiguousarray(weights[name], dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"{name}: shape {a.shape}, expected {shape}")
            keep[name] = a
            setattr(w, name, _ptr(a))
        for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
            if len(weights[name]) != d.L:
                raise ValueError(f"{name}: {len(weights[name])} layers, expected {d.L}")
            for l in range(L):
                a = np.ascontiguousarray(weights[name][l], dtype=np.float32)
                shape = {"w_ih": (d.Hp if l else d.D, H4), "w_hh": (d.Hp, H4)}.get(name, (H4,))
                if a.shape != shape:
                    raise ValueError(f"{name}[{l}]: shape {a.shape}, expected {shape}")
                keep[name, l] = a
                getattr(w, name)[l] = _ptr(a)
        self.weights = keep            # the fp32 arrays the handle was made from
        h = _vp()
        check(lib().asr_rnnt_create(ctypes.byref(desc), ctypes.byref(w), ctypes.byref(h)), "asr_rnnt_create")
        self.h = h.value
        self._work = None
        self._uploaded = False

    @classmethod
    def from_torch(cls, embedding, lstm, enc_proj, pred_proj, out_proj, blank: int, activation: str = "relu",
                   max_symbols: int = 10) -> "TransducerDecoder":
        """From torch.nn.Embedding, torch.nn.LSTM (unidirectional, with bias, no
        projection) and three torch.nn.Linear, transposed into [in][out]."""
        if lstm.bidirectional or not lstm.bias or getattr(lstm, "proj_size", 0):
            raise ValueError("the predictor is a unidirectional LSTM with bias and no projection")

        def arr(t):
            return t.detach().cpu().numpy().astype(np.float32)

        def lin(m):
            b = arr(m.bias) if m.bias is not None else np.zeros(m.out_features, np.float32)
            return np.ascontiguousarray(arr(m.weight).T), b

        L = lstm.num_layers
        wt = {"emb": arr(embedding.weight),
              "w_ih": [np.ascontiguousarray(arr(getattr(lstm, f"weight_ih_l{l}")).T) for l in range(L)],
              "w_hh": [np.ascontiguousarray(arr(getattr(lstm, f"weight_hh_l{l}")).T) for l in range(L)],
              "b_ih": [arr(getattr(lstm, f"bias_ih_l{l}")) for l in range(L)],
              "b_hh": [arr(getattr(lstm, f"bias_hh_l{l}")) for l in range(L)]}
        wt["w_enc"], wt["b_enc"] = lin(enc_proj)
        wt["w_pred"], wt["b_pred"] = lin(pred_proj)
        wt["w_out"], wt["b_out"] = lin(out_proj)
        d = rnnt_desc(embedding.num_embeddings, blank, enc_proj.in_features, embedding.embedding_dim,
                      lstm.hidden_size, L, enc_proj.out_features, activation, max_symbols)
        if lstm.input_size != d.D or pred_proj.in_features != d.Hp or pred_proj.out_features != d.J or \
                out_proj.in_features != d.J or out_proj.out_features != d.V:
            raise ValueError("the modules' sizes do not chain")
        return cls(d, wt)

    def info(self) -> dict:
        info = RnntInfo()
        check(lib().asr_rnnt_get_info(self.h, ctypes.byref(info)), "asr_rnnt_get_info")
        return {**{n: int(getattr(info.desc, n)) for n, _t in RnntDesc._fields_}, "uploaded": bool(info.uploaded),
                "lds_bytes": int(info.lds_bytes), "weight_bytes": int(info.weight_bytes)}

    def upload(self) -> None:
        """Copy the weights to the current device (synchronous; once)."""
        check(lib().asr_rnnt_upload(self.h), "asr_rnnt_upload")
        self._uploaded = True

    def workspace_bytes(self, T: int, B: int) -> int:
        return int(lib().asr_rnnt_workspace_bytes(self.h, T, B))

    def state_shape(self, B: int) -> tuple:
        """(2, L, B, Hp): h of every layer, then c."""
        return (2, int(self.desc.L), int(B), int(self.desc.Hp))

    def decode_device(self, d_enc: int, T: int, B: int, max_out: int, d_tokens: int, d_timesteps: int, d_logp: int,
                      d_count: int, d_total: int, d_work: int, d_lengths: int = 0, d_state_in: int = 0,
                      d_state_out: int = 0, stream: int = 0) -> None:
        """asr_rnnt_greedy on device pointers: asynchronous on stream."""
        check(lib().asr_rnnt_greedy(self.h, d_enc or None, d_lengths or None, T, B, max_out, d_state_in or None,
                                    d_state_out or None, d_tokens or None, d_timesteps or None, d_logp or None,
                                    d_count or None, d_total or None, d_work or None, stream or None),
              "asr_rnnt_greedy")

    @staticmethod
    def _unpack(B, max_out, tok, ts, lp, cnt, total):
        out = []
        for b in range(B):
            n = min(int(cnt[b]), max_out)
            out.append((tok[b, :n].tolist(), ts[b, :n].tolist(), lp[b, :n].copy(), float(total[b])))
        return out

    def _prepare(self, enc, lengths, max_out):
        enc = np.ascontiguousarray(enc, dtype=np.float32)
        if enc.ndim != 3 or enc.shape[2] != self.desc.E:
            raise ValueError(f"enc: shape {enc.shape}, expected (T, B, {self.desc.E})")
        T, B = enc.shape[0], enc.shape[1]
        if max_out is None:
            max_out = T * int(self.desc.max_symbols)
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        if ln is not None and ln.shape != (B,):
            raise ValueError(f"lengths: shape {ln.shape}, expected ({B},)")
        return enc, ln, T, B, int(max_out)

    def decode(self, enc, lengths=None, state=None, max_out=None, stream: int = 0):
        """enc [T, B, E] time-major.  Returns (results, state, counts): per
        utterance (tokens, timesteps, logps float64, total), the new state
        [2, L, B, Hp] float32 (pass it to the next chunk's decode and add the
        frame offset to the timesteps), and the emission counts int32 [B],
        which exceed max_out where records were dropped.  max_out defaults to
        T * max_symbols, the most a walk can emit."""
        enc, ln, T, B, max_out = self._prepare(enc, lengths, max_out)
        if not self._uploaded:
            self.upload()
        d_enc = _upload(enc, stream)
        d_len = _upload(ln, stream) if ln is not None else None
        shape = self.state_shape(B)
        nstate = int(np.prod(shape))
        d_sin = None
        if state is not None:
            st = np.ascontiguousarray(state, dtype=np.float32)
            if st.shape != shape:
                raise ValueError(f"state: shape {st.shape}, expected {shape}")
            d_sin = _upload(st, stream)
        d_sout = DeviceBytes(4 * nstate)
        mo = max(max_out, 1)
        d_tok, d_ts, d_lp = DeviceBytes(4 * B * mo), DeviceBytes(4 * B * mo), DeviceBytes(8 * B * mo)
        d_cnt, d_tot = DeviceBytes(max(4 * B, 16)), DeviceBytes(max(8 * B, 16))
        need = self.workspace_bytes(T, B)
        if self._work is None or self._work.nbytes < need:
            self._work = DeviceBytes(need)
        self.decode_device(d_enc.ptr, T, B, max_out, d_tok.ptr, d_ts.ptr, d_lp.ptr, d_cnt.ptr, d_tot.ptr,
                           self._work.ptr, d_len.ptr if d_len else 0, d_sin.ptr if d_sin else 0, d_sout.ptr, stream)
        check(lib().asr_stream_sync(stream or None), "asr_stream_sync")
        cnt = _download(d_cnt, (B,), np.int32, stream)
        total = _download(d_tot, (B,), np.float64, stream)
        tok = _download(d_tok, (B, mo), np.int32, stream)
        ts = _download(d_ts, (B, mo), np.int32, stream)
        lp = _download(d_lp, (B, mo), np.float64, stream)
        new_state = _download(d_sout, shape, np.float32, stream)
        return self._unpack(B, max_out, tok, ts, lp, cnt, total), new_state, cnt

    def decode_host(self, enc, lengths=None, state=None, max_out=None, gaps: bool = False):
        """The same through asr_rnnt_greedy_host (one thread, fp64): the state is
        float64; with gaps also the smallest top-2 logit gap of each
        utterance's walk."""
        enc, ln, T, B, max_out = self._prepare(enc, lengths, max_out)
        shape = self.state_shape(B)
        sin = None
        if state is not None:
            sin = np.ascontiguousarray(state, dtype=np.float64)
            if sin.shape != shape:
                raise ValueError(f"state: shape {sin.shape}, expected {shape}")
        sout = np.zeros(shape, np.float64)
        mo = max(max_out, 1)
        tok, ts, lp = np.zeros((B, mo), np.int32), np.zeros((B, mo), np.int32), np.zeros((B, mo), np.float64)
        cnt, total, gap = np.zeros(B, np.int32), np.zeros(B, np.float64), np.zeros(B, np.float64)
        check(lib().asr_rnnt_greedy_host(self.h, _ptr(enc), _ptr(ln) if ln is not None else None, T, B, max_out,
                                         _ptr(sin) if sin is not None else None, _ptr(sout), _ptr(tok), _ptr(ts),
                                         _ptr(lp), _ptr(cnt), _ptr(total), _ptr(gap) if gaps else None),
              "asr_rnnt_greedy_host")
        res = self._unpack(B, max_out, tok, ts, lp, cnt, total), sout, cnt
        return res + (gap,) if gaps else res

    # ---- beam search (asr_rnnt_beam*; the search is defined in include/asr_amd.h)
    def beam_workspace_bytes(self, T: int, B: int, beam: int) -> int:
        return int(lib().asr_rnnt_beam_workspace_bytes(self.h, T, B, beam))

    def _beam_prepare(self, enc, lengths, beam, nbest, max_out):
        enc, ln, T, B, _mo = self._prepare(enc, lengths, 0)
        nbest = int(beam) if nbest is None else int(nbest)
        max_out = T if max_out is None else int(max_out)    # one symbol per frame: at most T tokens
        return enc, ln, T, B, int(beam), nbest, max_out

    @staticmethod
    def _beam_unpack(B, max_out, tok, ts, ln, score, nhyp):
        out = []
        for b in range(B):
            hyps = []
            for j in range(int(nhyp[b])):
                n = min(int(ln[b, j]), max_out)
                hyps.append((tok[b, j, :n].tolist(), ts[b, j, :n].tolist(), float(score[b, j])))
            out.append(hyps)
        return out

    def beam_search_device(self, d_enc: int, T: int, B: int, beam: int, nbest: int, max_out: int, d_tokens: int,
                           d_timesteps: int, d_len: int, d_score: int, d_nhyp: int, d_work: int, d_lengths: int = 0,
                           stream: int = 0) -> None:
        """asr_rnnt_beam on device pointers: asynchronous on stream."""
        check(lib().asr_rnnt_beam(self.h, d_enc or None, d_lengths or None, T, B, beam, nbest, max_out,
                                  d_tokens or None, d_timesteps or None, d_len or None, d_score or None,
                                  d_nhyp or None, d_work or None, stream or None), "asr_rnnt_beam")

    # ---- LM fusion (asr_rnnt_lm_* / asr_rnnt_beam_lm*)
    def lm_tokens(self, lm: "NGramLM", tok_of_label=None) -> np.ndarray:
        """tok_of_label as int32 [V]; None: every label's string (self.labels)
        looked up in the model by name, -1 (an OOV) where it has none."""
        V = int(self.desc.V)
        if tok_of_label is None:
            if self.labels is None:
                raise ValueError("tok_of_label is required: the decoder has no labels")
            if len(self.labels) != V:
                raise ValueError(f"labels: {len(self.labels)} strings, expected {V}")
            tok_of_label = [-1 if v == self.desc.blank else lm.token_id(s) for v, s in enumerate(self.labels)]
        tok = np.ascontiguousarray(tok_of_label, dtype=np.int32)
        if tok.shape != (V,):
            raise ValueError(f"tok_of_label: shape {tok.shape}, expected ({V},)")
        return tok

    def _lm_handle(self, lm, alpha, beta, tok_of_label, bos, eos) -> int:
        """The fusion handle of (lm, weights, mapping, flags), made once and kept
        (with the LM) until close()."""
        tok = self.lm_tokens(lm, tok_of_label)
        flags = (ASR_LM_BOS if bos else 0) | (ASR_LM_EOS if eos else 0)
        key = (lm.h, float(np.float32(alpha)), float(np.float32(beta)), flags, tok.tobytes())
        if key not in self._fuse:
            z = _vp()
            check(lib().asr_rnnt_lm_create(self.h, lm.h, _ptr(tok), float(alpha), float(beta), flags, ctypes.byref(z)),
                  "asr_rnnt_lm_create")
            self._fuse[key] = (z.value, lm)
        return self._fuse[key][0]

    def beam_lm_workspace_bytes(self, fuse: int, T: int, B: int, beam: int) -> int:
        return int(lib().asr_rnnt_beam_lm_workspace_bytes(fuse, T, B, beam))

    @staticmethod
    def _beam_lm_unpack(B, max_out, tok, ts, ln, total, am, lml, ntok, nhyp):
        out = []
        for b in range(B):
            hyps = []
            for j in range(int(nhyp[b])):
                n = min(int(ln[b, j]), max_out)
                hyps.append((tok[b, j, :n].tolist(), ts[b, j, :n].tolist(), float(total[b, j]), float(am[b, j]),
                             float(lml[b, j]), int(ntok[b, j])))
            out.append(hyps)
        return out

    def beam_search_lm_device(self, fuse: int, d_enc: int, T: int, B: int, beam: int, nbest: int, max_out: int,
                              d_tokens: int, d_timesteps: int, d_len: int, d_total: int, d_nhyp: int, d_work: int,
                              d_am: int = 0, d_lm_log10: int = 0, d_ntok: int = 0, d_lengths: int = 0,
                              stream: int = 0) -> None:
        """asr_rnnt_beam_lm on device pointers: asynchronous on stream."""
        check(lib().asr_rnnt_beam_lm(fuse, d_enc or None, d_lengths or None, T, B, beam, nbest, max_out,
                                     d_tokens or None, d_timesteps or None, d_len or None, d_total or None,
                                     d_am or None, d_lm_log10 or None, d_ntok or None, d_nhyp or None,
                                     d_work or None, stream or None), "asr_rnnt_beam_lm")

    def _beam_search_lm(self, fuse, lm, enc, ln, T, B, beam, nbest, max_out, stream):
        if not self._uploaded:
            self.upload()
        lm.upload()
        d_enc = _upload(enc, stream)
        d_lens = _upload(ln, stream) if ln is not None else None
        mo, nb = max(max_out, 1), max(nbest, 1)
        d_tok, d_ts = DeviceBytes(4 * B * nb * mo), DeviceBytes(4 * B * nb * mo)
        d_len, d_nt, d_nh = DeviceBytes(max(4 * B * nb, 16)), DeviceBytes(max(4 * B * nb, 16)), DeviceBytes(max(4 * B, 16))
        d_tot, d_am, d_lml = (DeviceBytes(max(8 * B * nb, 16)) for _ in range(3))
        need = self.beam_lm_workspace_bytes(fuse, T, B, beam)
        if need and (self._work is None or self._work.nbytes < need):
            self._work = DeviceBytes(need)
        self.beam_search_lm_device(fuse, d_enc.ptr, T, B, beam, nbest, max_out, d_tok.ptr, d_ts.ptr, d_len.ptr,
                                   d_tot.ptr, d_nh.ptr, self._work.ptr if self._work else 0, d_am.ptr, d_lml.ptr,
                                   d_nt.ptr, d_lens.ptr if d_lens else 0, stream)
        check(lib().asr_stream_sync(stream or None), "asr_stream_sync")
        nhyp = _download(d_nh, (B,), np.int32, stream)
        hl = _download(d_len, (B, nb), np.int32, stream)
        nt = _download(d_nt, (B, nb), np.int32, stream)
        tot, am, lml = (_download(d, (B, nb), np.float64, stream) for d in (d_tot, d_am, d_lml))
        tok = _download(d_tok, (B, nb, mo), np.int32, stream)
        ts = _download(d_ts, (B, nb, mo), np.int32, stream)
        return self._beam_lm_unpack(B, max_out, tok, ts, hl, tot, am, lml, nt, nhyp)

    def lm_rescore(self, nbest, lm: "NGramLM", alpha: float, beta: float, tok_of_label=None, bos: bool = True,
                   eos: bool = False, host: bool = False, stream: int = 0):
        """An n-best of beam_search (without lm) re-ranked after the fact, as
        CTCDecoder.lm_rescore does: per utterance [(tokens, timesteps, total, am,
        lm_log10, n_tokens)], total descending (equal totals keep their order),
            total = am + alpha * ln(10) * lm_log10 + beta * n_tokens,
        am the hypothesis's score, lm_log10 asr_lm_score's value of its tokens
        (one launch for the whole batch; host=True: asr_lm_score_host)."""
        tok = self.lm_tokens(lm, tok_of_label)
        rows = [[int(tok[y]) for y in h[0]] for u in nbest for h in u]
        if not rows:
            return [[] for _ in nbest]
        if not host:
            lm.upload()
        lm_log10, counts = lm.score(rows, bos=bos, eos=eos, host=host, stream=stream)
        out, k = [], 0
        for u in nbest:
            res = []
            for h in u:
                n = int(counts[k, 0]) - (1 if eos else 0)
                res.append((h[0], h[1], lm_total(float(h[2]), float(lm_log10[k]), n, alpha, beta), float(h[2]),
                            float(lm_log10[k]), n))
                k += 1
            out.append(sorted(res, key=lambda r: -r[2]))
        return out

    def beam_search(self, enc, lengths=None, beam: int = 4, nbest=None, max_out=None, stream: int = 0, lm=None,
                    alpha: float = 0.0, beta: float = 0.0, tok_of_label=None, bos: bool = True, eos: bool = False):
        """One-symbol-per-frame beam search of width `beam` (1..16), one launch.
        enc [T, B, E] time-major.  Returns per utterance a list of (tokens,
        timesteps, score), best first, at most nbest (default: beam) of them;
        tokens and timesteps are cut at max_out (default T, the most a search
        can emit).  The token lists go into nbest_mbr and edit_distance as they
        are.  desc.max_symbols plays no part.
        With lm (an NGramLM) the model takes part in every prune with the
        weights alpha and beta (include/asr_amd.h has the definition) and a
        hypothesis is (tokens, timesteps, total, am, lm_log10, n_tokens);
        tok_of_label [V] maps labels to LM tokens (None: by the decoder's label
        strings), bos / eos are ASR_LM_BOS / ASR_LM_EOS."""
        enc, ln, T, B, beam, nbest, max_out = self._beam_prepare(enc, lengths, beam, nbest, max_out)
        if lm is not None:
            fuse = self._lm_handle(lm, alpha, beta, tok_of_label, bos, eos)
            return self._beam_search_lm(fuse, lm, enc, ln, T, B, beam, nbest, max_out, stream)
        if not self._uploaded:
            self.upload()
        d_enc = _upload(enc, stream)
        d_lens = _upload(ln, stream) if ln is not None else None
        mo, nb = max(max_out, 1), max(nbest, 1)
        d_tok, d_ts = DeviceBytes(4 * B * nb * mo), DeviceBytes(4 * B * nb * mo)
        d_len, d_sc, d_nh = DeviceBytes(max(4 * B * nb, 16)), DeviceBytes(max(8 * B * nb, 16)), DeviceBytes(max(4 * B, 16))
        need = self.beam_workspace_bytes(T, B, beam)
        if need and (self._work is None or self._work.nbytes < need):
            self._work = DeviceBytes(need)
        self.beam_search_device(d_enc.ptr, T, B, beam, nbest, max_out, d_tok.ptr, d_ts.ptr, d_len.ptr, d_sc.ptr,
                                d_nh.ptr, self._work.ptr if self._work else 0, d_lens.ptr if d_lens else 0, stream)
        check(lib().asr_stream_sync(stream or None), "asr_stream_sync")
        nhyp = _download(d_nh, (B,), np.int32, stream)
        hl = _download(d_len, (B, nb), np.int32, stream)
        sc = _download(d_sc, (B, nb), np.float64, stream)
        tok = _download(d_tok, (B, nb, mo), np.int32, stream)
        ts = _download(d_ts, (B, nb, mo), np.int32, stream)
        return self._beam_unpack(B, max_out, tok, ts, hl, sc, nhyp)

    def beam_search_host(self, enc, lengths=None, beam: int = 4, nbest=None, max_out=None, margins: bool = False,
                         lm=None, alpha: float = 0.0, beta: float = 0.0, tok_of_label=None, bos: bool = True,
                         eos: bool = False):
        """The same through asr_rnnt_beam_host (one thread, fp64); with margins
        also the smallest decision margin of each utterance's search (float64
        [B]; include/asr_amd.h says what counts).  With lm: asr_rnnt_beam_lm_host,
        the keywords and the hypotheses as in beam_search."""
        enc, ln, T, B, beam, nbest, max_out = self._beam_prepare(enc, lengths, beam, nbest, max_out)
        mo, nb = max(max_out, 1), max(nbest, 1)
        tok, ts = np.zeros((B, nb, mo), np.int32), np.zeros((B, nb, mo), np.int32)
        hl, sc, nhyp = np.zeros((B, nb), np.int32), np.zeros((B, nb), np.float64), np.zeros(B, np.int32)
        margin = np.zeros(B, np.float64)
        if lm is not None:
            fuse = self._lm_handle(lm, alpha, beta, tok_of_label, bos, eos)
            am, lml, nt = np.zeros((B, nb), np.float64), np.zeros((B, nb), np.float64), np.zeros((B, nb), np.int32)
            check(lib().asr_rnnt_beam_lm_host(fuse, _ptr(enc), _ptr(ln) if ln is not None else None, T, B, beam, nbest,
                                              max_out, _ptr(tok), _ptr(ts), _ptr(hl), _ptr(sc), _ptr(am), _ptr(lml),
                                              _ptr(nt), _ptr(nhyp), _ptr(margin) if margins else None),
                  "asr_rnnt_beam_lm_host")
            res = self._beam_lm_unpack(B, max_out, tok, ts, hl, sc, am, lml, nt, nhyp)
            return (res, margin) if margins else res
        check(lib().asr_rnnt_beam_host(self.h, _ptr(enc), _ptr(ln) if ln is not None else None, T, B, beam, nbest,
                                       max_out, _ptr(tok), _ptr(ts), _ptr(hl), _ptr(sc), _ptr(nhyp),
                                       _ptr(margin) if margins else None), "asr_rnnt_beam_host")
        res = self._beam_unpack(B, max_out, tok, ts, hl, sc, nhyp)
        return (res, margin) if margins else res

    # ---- lattice scoring and forced alignment (asr_rnnt_align*; defined in include/asr_amd.h)
    def align_workspace_bytes(self, T: int, B: int, N: int, max_target_len: int) -> int:
        return int(lib().asr_rnnt_align_workspace_bytes(self.h, T, B, N, max_target_len))

    def align_device(self, d_enc: int, T: int, B: int, d_targets: int, ldt: int, d_target_lengths: int, N: int,
                     max_target_len: int, topology: int, d_score: int, d_vscore: int, d_frames: int, d_work: int,
                     d_lengths: int = 0, d_utt: int = 0, stream: int = 0) -> None:
        """asr_rnnt_align on device pointers (0 = NULL): asynchronous on stream."""
        check(lib().asr_rnnt_align(self.h, d_enc or None, d_lengths or None, T, B, d_targets or None, ldt,
                                   d_target_lengths or None, d_utt or None, N, max_target_len, topology,
                                   d_score or None, d_vscore or None, d_frames or None, d_work or None,
                                   stream or None), "asr_rnnt_align")

    def _align_prepare(self, enc, targets, lengths, utt, topology, max_target_len):
        enc, ln, T, B, _mo = self._prepare(enc, lengths, 0)
        tg, tl, mtl = _pack_rows(targets)
        if max_target_len is not None:    # a wider table: the results do not depend on it
            mtl = int(max_target_len)
            wide = np.zeros((tg.shape[0], max(mtl, 1)), np.int32)
            k = min(wide.shape[1], tg.shape[1])
            wide[:, :k] = tg[:, :k]
            tg = wide
        N = len(targets)
        ut = None
        if utt is not None:
            ut = np.ascontiguousarray(utt, dtype=np.int32)
            if ut.shape != (N,):
                raise ValueError(f"utt: shape {ut.shape}, expected ({N},)")
        topo = RNNT_TOPOLOGIES[topology] if isinstance(topology, str) else int(topology)
        return enc, ln, T, B, tg, tl, mtl, N, ut, topo

    def _align(self, enc, targets, lengths, utt, topology, stream, want, max_target_len=None):
        """want = (score, vscore, frames): which outputs are asked for."""
        enc, ln, T, B, tg, tl, mtl, N, ut, topo = self._align_prepare(enc, targets, lengths, utt, topology,
                                                                      max_target_len)
        if not self._uploaded:
            self.upload()
        ldt = tg.shape[1]
        d_enc, d_tg, d_tl = _upload(enc, stream), _upload(tg, stream), _upload(tl, stream)
        d_len = _upload(ln, stream) if ln is not None else None
        d_utt = _upload(ut, stream) if ut is not None else None
        d_sc = DeviceBytes(max(8 * N, 16)) if want[0] else None
        d_vs = DeviceBytes(max(8 * N, 16)) if want[1] else None
        d_fr = DeviceBytes(max(4 * N * ldt, 16)) if want[2] else None
        need = self.align_workspace_bytes(T, B, N, mtl)
        if need and (self._work is None or self._work.nbytes < need):
            self._work = DeviceBytes(need)
        self.align_device(d_enc.ptr, T, B, d_tg.ptr, ldt, d_tl.ptr, N, mtl, topo, d_sc.ptr if d_sc else 0,
                          d_vs.ptr if d_vs else 0, d_fr.ptr if d_fr else 0, self._work.ptr if self._work else 0,
                          d_len.ptr if d_len else 0, d_utt.ptr if d_utt else 0, stream)
        check(lib().asr_stream_sync(stream or None), "asr_stream_sync")
        score = _download(d_sc, (N,), np.float64, stream) if want[0] else None
        vscore = _download(d_vs, (N,), np.float64, stream) if want[1] else None
        frames = None
        if want[2]:
            fr = _download(d_fr, (N, ldt), np.int32, stream)
            frames = [fr[n, :min(len(targets[n]), mtl)].copy() for n in range(N)]
        return score, vscore, frames

    def _align_host(self, enc, targets, lengths, utt, topology, want):
        enc, ln, T, B, tg, tl, mtl, N, ut, topo = self._align_prepare(enc, targets, lengths, utt, topology, None)
        ldt = tg.shape[1]
        score = np.zeros(N, np.float64) if want[0] else None
        vscore = np.zeros(N, np.float64) if want[1] else None
        fr = np.zeros((N, ldt), np.int32) if want[2] else None
        check(lib().asr_rnnt_align_host(self.h, _ptr(enc), _ptr(ln) if ln is not None else None, T, B, _ptr(tg), ldt,
                                        _ptr(tl), _ptr(ut) if ut is not None else None, N, mtl, topo,
                                        _ptr(score) if want[0] else None, _ptr(vscore) if want[1] else None,
                                        _ptr(fr) if want[2] else None), "asr_rnnt_align_host")
        frames = [fr[n, :len(targets[n])].copy() for n in range(N)] if want[2] else None
        return score, vscore, frames

    def score(self, enc, targets: Sequence[Sequence[int]], lengths=None, utt=None, topology="standard",
              stream: int = 0) -> np.ndarray:
        """Exact transducer log-likelihood log p(target | enc) of every target,
        fp64 [N] (-inf: infeasible).  enc [T, B, E] time-major; targets: a list
        of label lists, target n scored against utterance utt[n] (default n);
        topology "standard" (a label arc stays in the frame: the training
        lattice) or "one_per_frame" (the lattice beam_search searches)."""
        return self._align(enc, targets, lengths, utt, topology, stream, (True, False, False))[0]

    def align(self, enc, targets: Sequence[Sequence[int]], lengths=None, utt=None, topology="standard",
              stream: int = 0):
        """(score, vscore, frames): the forward score, the log-probability of the
        best alignment and, per target, the frame at which that alignment emits
        each label (int32 [U_n]; -1 when the target is infeasible), the
        convention of decode's and beam_search's timesteps."""
        return self._align(enc, targets, lengths, utt, topology, stream, (True, True, True))

    def score_host(self, enc, targets, lengths=None, utt=None, topology="standard") -> np.ndarray:
        """score through asr_rnnt_align_host (one thread, fp64)."""
        return self._align_host(enc, targets, lengths, utt, topology, (True, False, False))[0]

    def align_host(self, enc, targets, lengths=None, utt=None, topology="standard"):
        """align through asr_rnnt_align_host (one thread, fp64)."""
        return self._align_host(enc, targets, lengths, utt, topology, (True, True, True))

    def rescore(self, nbest, enc, lengths=None, topology="one_per_frame", stream: int = 0, host: bool = False):
        """An n-best of beam_search re-ranked by the exact score, as
        CTCDecoder.rescore does: per utterance [(tokens, search_score,
        exact_score)], exact score descending (equal scores keep the search
        order).  A search score sums only the alignments that survived the
        width-K prune, a lower bound; the exact one is asr_rnnt_align's forward
        score of every hypothesis against its utterance, one call for the whole
        batch (N = sum of K, utt[n] = the utterance; host=True: through
        asr_rnnt_align_host).  The exact scores go into
        nbest_mbr(log_weights_per_utt=...) as they are."""
        targets = [list(h[0]) for u in nbest for h in u]
        utt = [b for b, u in enumerate(nbest) for _ in u]
        if not targets:
            return [[] for _ in nbest]
        if host:
            exact = self.score_host(enc, targets, lengths=lengths, utt=utt, topology=topology)
        else:
            exact = self.score(enc, targets, lengths=lengths, utt=utt, topology=topology, stream=stream)
        out, k = [], 0
        for u in nbest:
            rows = [(list(h[0]), float(h[2]), float(exact[k + j])) for j, h in enumerate(u)]
            k += len(u)
            out.append(sorted(rows, key=lambda r: -r[2]))
        return out

    def close(self) -> None:
        for z, _lm in getattr(self, "_fuse", {}).values():
            lib().asr_rnnt_lm_destroy(z)
        self._fuse = {}
        if self.h:
            lib().asr_rnnt_destroy(self.h)
            self.h = None
        self._work = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------ edit distance, WER and n-best MBR rescoring
ASR_EDIT_MAX_LEN = 1024
ASR_MBR_MAX_HYPS = 256


def _pack_rows(rows: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray, int]:
    """Token lists as (table [n][ld] int32, lengths [n], longest length)."""
    max_len = max([len(r) for r in rows] + [0])
    tab = np.zeros((len(rows), max(max_len, 1)), np.int32)
    for n, r in enumerate(rows):
        tab[n, :len(r)] = np.asarray(r, dtype=np.int32)
    return tab, np.array([len(r) for r in rows], np.int32), max_len


def edit_distance(refs: Sequence[Sequence[int]], hyps: Sequence[Sequence[int]], pairs=None, detail: bool = False,
                  host: bool = False, stream: int = 0):
    """Levenshtein distance of token lists (the semantics are in
    include/asr_amd.h): int32 [P]; with detail also the [P, 4] counts (hits,
    substitutions, deletions, insertions) of the alignment the tie rule fixes.
    Pair p is (refs[p], hyps[p]), or (refs[i], hyps[j]) for pairs[p] = (i, j);
    an index outside its list gives -1.  host=True runs asr_edit_distance_host;
    otherwise one asr_edit_distance launch on stream."""
    if pairs is None:
        if len(refs) != len(hyps):
            raise ValueError("edit_distance: refs and hyps differ in number and no pairs are given")
        P, ri, hi = len(refs), None, None
    else:
        idx = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        P, ri, hi = len(idx), np.ascontiguousarray(idx[:, 0]), np.ascontiguousarray(idx[:, 1])
    if P == 0:
        return (np.zeros(0, np.int32), np.zeros((0, 4), np.int32)) if detail else np.zeros(0, np.int32)
    rt, rl, rmax = _pack_rows(refs)
    ht, hl, hmax = _pack_rows(hyps)
    dist = np.zeros(P, np.int32)
    ops = np.zeros((P, 4), np.int32) if detail else None
    if host:
        check(lib().asr_edit_distance_host(_ptr(rt), rt.shape[1], _ptr(rl), len(refs), rmax, _ptr(ht), ht.shape[1],
                                           _ptr(hl), len(hyps), hmax, None if ri is None else _ptr(ri),
                                           None if hi is None else _ptr(hi), P, _ptr(dist),
                                           _ptr(ops) if detail else None), "asr_edit_distance_host")
    else:
        d_rt, d_rl, d_ht, d_hl = (_upload(a, stream) for a in (rt, rl, ht, hl))
        d_ri = None if ri is None else _upload(ri, stream)
        d_hi = None if hi is None else _upload(hi, stream)
        d_dist = DeviceBytes(4 * P)
        d_ops = DeviceBytes(16 * P) if detail else None
        check(lib().asr_edit_distance(d_rt.ptr, rt.shape[1], d_rl.ptr, len(refs), rmax, d_ht.ptr, ht.shape[1],
                                      d_hl.ptr, len(hyps), hmax, d_ri.ptr if d_ri else None,
                                      d_hi.ptr if d_hi else None, P, d_dist.ptr, d_ops.ptr if detail else None,
                                      stream or None), "asr_edit_distance")
        dist = _download(d_dist, P, np.int32, stream)
        ops = _download(d_ops, (P, 4), np.int32, stream) if detail else None
    return (dist, ops) if detail else dist


def wer(refs: Sequence[Sequence[int]], hyps: Sequence[Sequence[int]], host: bool = False) -> dict:
    """Corpus error rate of hyps[p] against refs[p] over tokens (labels: CER,
    word ids from word_tokens: WER): errors, ref_tokens, hits, sub, del, ins and
    wer = errors / ref_tokens (inf for errors against no reference token, 0.0
    for none of either)."""
    _, ops = edit_distance(refs, hyps, detail=True, host=host)
    h, s, d, i = (int(x) for x in ops.astype(np.int64).sum(axis=0)) if len(ops) else (0, 0, 0, 0)
    errors, ref_tokens = s + d + i, h + s + d
    rate = errors / ref_tokens if ref_tokens else (math.inf if errors else 0.0)
    return {"errors": errors, "ref_tokens": ref_tokens, "hits": h, "sub": s, "del": d, "ins": i, "wer": rate}


def word_tokens(label_lists: Sequence[Sequence[int]], labels: Sequence[str], space: str = " ") -> List[List[int]]:
    """Hypotheses of label ids as lists of word ids: the label strings are joined,
    split at `space`, and every non-empty word gets an id from one dictionary
    that grows over the call (first seen, first numbered), so that references
    and hypotheses passed together share their ids."""
    labels = list(labels)
    ids: dict = {}
    return [[ids.setdefault(w, len(ids)) for w in "".join(labels[c] for c in hyp).split(space) if w != ""]
            for hyp in label_lists]


def nbest_mbr(token_lists_per_utt: Sequence[Sequence[Sequence[int]]], log_weights_per_utt=None, host: bool = False,
              stream: int = 0):
    """Minimum-Bayes-risk scores of n-best lists (asr_nbest_mbr): per utterance
    the hypotheses' token lists and their natural-log weights (None: uniform).
    Returns (risks: a float64 array per utterance, best: int32 [utterances], the
    index of the smallest risk, -1 for an empty list; distances: an int32 [n, n]
    matrix per utterance).  host=True runs asr_nbest_mbr_host; otherwise one
    asr_nbest_mbr call (two launches) on stream."""
    G = len(token_lists_per_utt)
    sizes = [len(u) for u in token_lists_per_utt]
    N = sum(sizes)
    if N == 0:
        return [np.zeros(0, np.float64) for _ in sizes], np.full(G, -1, np.int32), \
            [np.zeros((0, 0), np.int32) for _ in sizes]
    tok, ln, max_len = _pack_rows([t for u in token_lists_per_utt for t in u])
    gs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    max_hyps = max(sizes)
    w = None
    if log_weights_per_utt is not None:
        w = np.ascontiguousarray([x for u in log_weights_per_utt for x in u], dtype=np.float64)
        if w.shape != (N,):
            raise ValueError("nbest_mbr: one weight per hypothesis")
    dist = np.zeros((N, max_hyps), np.int32)
    risk, best = np.zeros(N, np.float64), np.zeros(G, np.int32)
    if host:
        check(lib().asr_nbest_mbr_host(_ptr(tok), tok.shape[1], _ptr(ln), N, max_len, _ptr(gs), G, max_hyps,
                                       None if w is None else _ptr(w), _ptr(dist), max_hyps, _ptr(risk), _ptr(best)),
              "asr_nbest_mbr_host")
    else:
        d_tok, d_ln, d_gs = _upload(tok, stream), _upload(ln, stream), _upload(gs, stream)
        d_w = None if w is None else _upload(w, stream)
        d_dist, d_risk, d_best = DeviceBytes(4 * N * max_hyps), DeviceBytes(8 * N), DeviceBytes(max(4 * G, 16))
        check(lib().asr_nbest_mbr(d_tok.ptr, tok.shape[1], d_ln.ptr, N, max_len, d_gs.ptr, G, max_hyps,
                                  d_w.ptr if d_w else None, d_dist.ptr, max_hyps, d_risk.ptr, d_best.ptr,
                                  stream or None), "asr_nbest_mbr")
        dist = _download(d_dist, (N, max_hyps), np.int32, stream)
        risk = _download(d_risk, N, np.float64, stream)
        best = _download(d_best, G, np.int32, stream)
    return ([risk[gs[g]:gs[g + 1]].copy() for g in range(G)], best,
            [dist[gs[g]:gs[g + 1], :sizes[g]].copy() for g in range(G)])


class PipelineConfig(ctypes.Structure):
    """asr_pipeline_config (include/asr_amd.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("T", "B", "in_", "H", "V", "beam", "blank", "inflight",
                                           "prod_streams", "decode_cus", "segments")]


PIPELINE_MODES = {0: "CU groups (small batches)", 1: "chip-filling batches", 2: "CU groups (H > 256)"}


def model_emissions(x: "DeviceMatrix", weights, T: int, B: int, emis: "DeviceMatrix", fused: bool,
                    work: Optional["DeviceMatrix"] = None, stream: int = 0,
                    recurrence: Optional[int] = None) -> "DeviceMatrix":
    """One batch's emissions the way a Pipeline produces them
    (asr_pipeline_get_production): fused — input projection GEMM, then the
    recurrence with the emission layer fused (asr_rnn_emit_fwd); otherwise
    asr_rnn_fwd then asr_linear_fwd(..., log_softmax), with the recurrence
    kind the pipeline pinned (`recurrence`, Pipeline.describe()["recurrence"];
    None / AUTO: the process-wide choice), restored afterwards.  weights =
    (W_ih, W_hh, b_ih, b_hh, W_out, b_out); work [T*B, H] is scratch
    (allocated if None)."""
    W_ih, W_hh, b_ih, b_hh, W_out, b_out = weights
    work = work if work is not None else DeviceMatrix(T * B, W_hh.cols)
    if fused:
        linear_fwd(x, W_ih, None, work, EPI_NONE, stream)
        rnn_emit_fwd(W_hh, b_ih, b_hh, W_out, b_out, work, emis, T, B, stream=stream)
        return emis
    prev = None
    if recurrence not in (None, RNN_RECUR_AUTO):
        prev = rnn_get_recurrence()
        rnn_set_recurrence(recurrence)
    try:
        rnn_fwd(x, W_ih, W_hh, b_ih, b_hh, work, T, B, stream=stream)
    finally:
        if prev is not None:
            rnn_set_recurrence(prev)
    linear_fwd(work, W_out, b_out, emis, EPI_BIAS_LOGSOFTMAX, stream)
    return emis


class Pipeline:
    """asr_pipeline_*: RNN -> Linear + log_softmax -> CTC decode over a stream of
    equal-shape batches, the library overlapping production and decodes on its
    own streams.  submit(x) queues a batch (features stay valid until its
    results are collected); collect() returns the oldest batch's
    (labels [B][T], lengths [B], logp [B], decode_ms)."""

    def __init__(self, T: int, B: int, inp: int, H: int, V: int, beam: int, weights, blank: int = 0,
                 inflight: int = 0, prod_streams: int = 0, decode_cus: int = 0, segments: int = 0,
                 coalesce: int = 1):
        """coalesce > 1: dynamic batching (asr_pipeline_create_coalesced):
        `coalesce` consecutive submits of B utterances run as one batch; the
        schedule (inflight, prod_streams, ...) is that batch's."""
        self.T, self.B = T, B
        self.coalesce = max(1, int(coalesce))
        self.cfg = PipelineConfig(T, B, inp, H, V, beam, blank, inflight, prod_streams, decode_cus, segments)
        self._w = weights   # (W_ih, W_hh, b_ih, b_hh, W_out, b_out) DeviceMatrix: kept alive
        h = _vp()
        if self.coalesce > 1:
            check(lib().asr_pipeline_create_coalesced(ctypes.byref(self.cfg), self.coalesce,
                                                      *[w.ptr for w in weights], ctypes.byref(h)),
                  "asr_pipeline_create_coalesced")
        else:
            check(lib().asr_pipeline_create(ctypes.byref(self.cfg), *[w.ptr for w in weights], ctypes.byref(h)),
                  "asr_pipeline_create")
        self.h = h.value
        self._lab = np.zeros((B, max(T, 1)), np.int32)
        self._len = np.zeros(B, np.int32)
        self._lp = np.zeros(B, np.float64)
        self._inputs = collections.deque()   # submitted features, alive until their batch is collected
        self._kept = []                      # features of failed submits (alive until close)

    def describe(self):
        m, d, p, c, w = _i(), _i(), _i(), _i(), _i()
        check(lib().asr_pipeline_describe(self.h, ctypes.byref(m), ctypes.byref(d), ctypes.byref(p),
                                          ctypes.byref(c), ctypes.byref(w)), "asr_pipeline_describe")
        fz, gr, rk = _i(), ctypes.c_longlong(), _i()
        check(lib().asr_pipeline_get_production(self.h, ctypes.byref(fz), ctypes.byref(gr), ctypes.byref(rk)),
              "asr_pipeline_get_production")
        ns, hq, sg, gp = _i(), _i(), _i(), _i()
        check(lib().asr_pipeline_get_streams(self.h, ctypes.byref(ns), ctypes.byref(hq)), "asr_pipeline_get_streams")
        check(lib().asr_pipeline_get_segments(self.h, ctypes.byref(sg)), "asr_pipeline_get_segments")
        check(lib().asr_pipeline_get_groups(self.h, ctypes.byref(gp)), "asr_pipeline_get_groups")
        qs, qd = _i(), _i()
        check(lib().asr_pipeline_get_queue_use(self.h, ctypes.byref(qs), ctypes.byref(qd)),
              "asr_pipeline_get_queue_use")
        hb, f0 = _i(), ctypes.c_double()
        check(lib().asr_pipeline_get_drain(self.h, ctypes.byref(hb), ctypes.byref(f0)), "asr_pipeline_get_drain")
        return {"mode": PIPELINE_MODES.get(m.value, m.value), "inflight": d.value, "prod_streams": p.value,
                "decode_cus": c.value, "decode_waves": w.value, "fused_emission": bool(fz.value),
                "decode_cu_gemm_rows": gr.value, "recurrence": rk.value, "streams": ns.value,
                "hw_queues": hq.value, "segments": sg.value, "groups": gp.value,
                "drain_held_batches": hb.value, "first_segment_share": round(f0.value, 4),
                "shared_queue_streams": qs.value, "dedicated_queue_streams": qd.value,
                "coalesce": self.coalesce}

    def placement(self):
        """[(role name, cu_lo, cu_hi)] of every stream the pipeline created."""
        n = _i()
        check(lib().asr_pipeline_get_placement(self.h, 0, ctypes.byref(n), None, None, None),
              "asr_pipeline_get_placement")
        cnt = n.value
        role, lo, hi = (_i * max(1, cnt))(), (_i * max(1, cnt))(), (_i * max(1, cnt))()
        check(lib().asr_pipeline_get_placement(self.h, cnt, ctypes.byref(n), role, lo, hi),
              "asr_pipeline_get_placement")
        return [(PIPE_ROLES.get(role[i], role[i]), lo[i], hi[i]) for i in range(cnt)]

    def probe_placement(self, role: str):
        """Physical CUs per XCD that the first stream of `role` reaches (one
        probe launch; synchronises that stream): a list, one count per XCD."""
        r = {v: k for k, v in PIPE_ROLES.items()}[role]
        cnt, nx = (_i * ASR_MAX_XCC)(), _i()
        check(lib().asr_pipeline_probe_placement(self.h, r, cnt, ctypes.byref(nx)), "asr_pipeline_probe_placement")
        return [cnt[i] for i in range(nx.value)]

    def set_timing(self, on: bool = True) -> None:
        """Record per-batch production / decode timing events from the next
        submit on (call on a drained pipeline; clears the timeline)."""
        check(lib().asr_pipeline_set_timing(self.h, 1 if on else 0), "asr_pipeline_set_timing")

    def timeline(self):
        """(batch ids [n], stamps [n, 4] ms: production start / end, decode
        start / end) of the batches collected since set_timing."""
        n = _i()
        check(lib().asr_pipeline_get_timeline(self.h, 0, ctypes.byref(n), None, None), "asr_pipeline_get_timeline")
        cnt = n.value
        b = np.zeros(max(1, cnt), np.int64)
        t = np.zeros((max(1, cnt), 4), np.float32)
        check(lib().asr_pipeline_get_timeline(self.h, cnt, ctypes.byref(n),
                                              b.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                              t.ctypes.data_as(ctypes.POINTER(_f))), "asr_pipeline_get_timeline")
        return b[:cnt], t[:cnt]

    def submit(self, x: "DeviceMatrix") -> None:
        """Queue a batch.  x is kept alive here until its batch is collected
        (asr_pipeline_submit reads it until then); after a failed submit it
        is kept until close(): queued work of the batch may still read it."""
        rc = lib().asr_pipeline_submit(self.h, x.ptr)
        if rc != ASR_OK:
            self._kept.append(x)
            check(rc, "asr_pipeline_submit")
        self._inputs.append(x)

    def pending(self) -> int:
        n = _i()
        check(lib().asr_pipeline_pending(self.h, ctypes.byref(n)), "asr_pipeline_pending")
        return n.value

    def collect(self, out=None):
        """(labels [B][T] int32, lengths [B], logp [B] fp64, decode_ms) of the
        oldest batch; the arrays are reused by the next call unless the caller
        passes its own (out = (labels, lengths, logp) of those shapes / dtypes)."""
        ms = _f()
        lab, ln, lp = (self._lab, self._len, self._lp) if out is None else out
        assert lab.dtype == np.int32 and lab.shape == self._lab.shape and lab.flags.c_contiguous
        assert ln.dtype == self._len.dtype and ln.shape == self._len.shape
        assert lp.dtype == np.float64 and lp.shape == self._lp.shape
        rc = lib().asr_pipeline_collect(self.h, _ptr(lab), lab.shape[1], _ptr(ln), _ptr(lp), ctypes.byref(ms))
        n = _i()
        if lib().asr_pipeline_pending(self.h, ctypes.byref(n)) == ASR_OK:
            while len(self._inputs) > n.value:   # collected batches' features may go
                self._inputs.popleft()
        check(rc, "asr_pipeline_collect")
        return lab, ln, lp, ms.value

    def peek_emissions(self) -> np.ndarray:
        """Host copy of the emissions [T][B][V] the last collected batch's
        decode consumed (asr_pipeline_peek_emissions)."""
        ptr = _vp()
        check(lib().asr_pipeline_peek_emissions(self.h, ctypes.byref(ptr)), "asr_pipeline_peek_emissions")
        g, col = self.coalesce, _i()
        if g > 1:   # the whole coalesced batch, then this submit's columns
            check(lib().asr_pipeline_get_coalesce(self.h, None, None, ctypes.byref(col)), "asr_pipeline_get_coalesce")
        out = np.empty((self.T, g * self.B, self.cfg.V), np.float32)
        check(lib().asr_memcpy_d2h(_ptr(out), ptr.value, out.nbytes, None), "asr_memcpy_d2h")
        if g > 1:
            out = np.ascontiguousarray(out[:, col.value * self.B:(col.value + 1) * self.B, :])
        return out

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().asr_pipeline_destroy(self.h)   # synchronises the pipeline's streams
            self.h = None
        self._inputs = collections.deque()
        self._kept = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CTCBeamSearch:
    """CTCBeamSearch.h:107 — CTCBeamSearch(vocab, vocabSize, beamWidth, blankID).

    decode(seqProb, timestep, batchSize) takes probabilities [T*B, V]
    (time-major rows, CTCBeamSearch.cu:67-69) and returns, per utterance, the
    best string and its probability as float (cu:283-298); `logprobs` holds
    the fp64 log-probabilities of the last decode.
    """

    def __init__(self, vocab: Sequence[str], vocabSize: int, beamWidth: int, blankID: int):
        self.vocab = [str(c) for c in list(vocab)[:vocabSize]]
        self.vocabSize, self.beamWidth, self.blankID = vocabSize, beamWidth, blankID
        codes = [ord(c) & 0xFF if len(c) == 1 else i for i, c in enumerate(self.vocab)]
        self._dec = CTCDecoder(vocabSize, beamWidth, blankID, codes)
        self.logprobs: Optional[np.ndarray] = None

    def decode(self, seqProb: np.ndarray, timestep: int, batchSize: int) -> List[Tuple[str, float]]:
        seqProb = np.asarray(seqProb, np.float32)
        if seqProb.shape[-1] != self.vocabSize:
            raise ValueError("Error: inconsistent vocabulary size in CTC decoder")
        self._dec.decode(seqProb.reshape(timestep, batchSize, self.vocabSize), is_log=False)
        labels, lp = self._dec.best()
        self.logprobs = lp
        return [("".join(self.vocab[i] for i in lab), float(np.exp(l))) for lab, l in zip(labels, lp)]


class CTCBeamDecoder:
    """Batch interface of the Python baseline's decoder (baseline/main.py:10,
    29, 46: ctcdecode.CTCBeamDecoder(labels, beam_width=, blank_id=,
    num_processes=, log_probs_input=True).decode(probs[B,T,V], seq_lens)) on
    this library's decoder.  ctcdecode itself is not available here, so the
    search semantics are the reference C++ decoder's (CTCBeamSearch.cpp with
    F1-F3), not ctcdecode's.  decode returns (beam_results [B, beam_width, T] int32 label
    ids, beam_scores [B, beam_width] float32 = -log p (lower is better),
    timesteps [B, beam_width, T] int32, out_lens [B, beam_width] int32);
    hypotheses beyond an utterance's final beam have length 0 and score +inf.
    timesteps[b, k, i] is the frame at which label i of hypothesis k was
    FIRST APPENDED in the surviving search lineage (asr_ctc_set_timesteps).
    This differs from ctcdecode, which reports the frame of its trie node's
    best emission; the two are not pinned against each other (ctcdecode is
    unavailable here).  -1 past a hypothesis' length.  Tracking costs a second
    node table per decode, so it is on only with timesteps=True (the
    default, as ctcdecode always returns them); timesteps=False returns an
    all -1 array and decodes on the plain path.  probs may be a numpy array
    or a torch tensor (a GPU tensor is decoded in place, no copy).

    With model_path (an ARPA file of a character, BPE or word-piece model whose
    tokens are the label strings) the search is CTCLMDecoder's: the LM is fused
    into every prune with alpha and beta, <s> as the first context and no
    </s>, top_n = cutoff_top_n.  Every label is mapped to a token by
    NGramLM.label_tokens; if no non-blank label is a token (a word-level
    model) ValueError is raised: use CTCDecoder.lm_rescore with
    NGramLM.label_mapper(labels, mode="word") instead.  beam_scores is then
    -total (total = ctc + alpha ln10 lm_log10 + beta n_tokens) and timesteps is
    all -1 (the fused search records none).  cutoff_prob other than 1.0 is not
    implemented with a model (NotImplementedError).  Without model_path,
    cutoff_top_n, cutoff_prob, alpha and beta are ignored, as before.

    With lexicon="open" or "closed" model_path is a word-level model: its
    tokens are spelled in the labels (Lexicon.from_lm, `space` the label that
    separates words) and the search is CTCLMDecoder.word's, the LM term added
    when a word ends; "closed" keeps the search inside the lexicon.  The same
    outputs as with a label-level model.  ValueError if `space` is not a
    label.  lexicon=None changes nothing."""

    def __init__(self, labels: Sequence[str], model_path: Optional[str] = None, alpha: float = 0.0,
                 beta: float = 0.0, cutoff_top_n: int = 40, cutoff_prob: float = 1.0,
                 beam_width: int = 100, num_processes: int = 4, blank_id: int = 0,
                 log_probs_input: bool = False, timesteps: bool = True, lexicon: Optional[str] = None,
                 space: str = " "):
        self.labels = list(labels)
        self.beam_width, self.blank_id, self.log_probs_input = beam_width, blank_id, log_probs_input
        self.track_timesteps = bool(timesteps)
        self._lm: Optional[NGramLM] = None
        self._lex: Optional[Lexicon] = None
        self._fused: Optional[CTCLMDecoder] = None
        self._dec: Optional[CTCDecoder] = None
        if lexicon is not None:
            if lexicon not in ("open", "closed"):
                raise ValueError(f"lexicon {lexicon!r}: None, \"open\" or \"closed\"")
            if model_path is None:
                raise ValueError("lexicon needs model_path, a word-level ARPA model")
            if space not in self.labels:
                raise ValueError(f"lexicon: the space {space!r} is not a label")
        if model_path is not None:
            if cutoff_prob != 1.0:
                raise NotImplementedError("cutoff_prob other than 1.0 is not implemented with a language model")
            self._lm = NGramLM.from_arpa(model_path)
            if lexicon is not None:
                self._lex = Lexicon.from_lm(self._lm, self.labels, space, blank_id)
                self._fused = CTCLMDecoder.word(len(self.labels), beam_width, self._lm, self._lex, alpha, beta,
                                                blank_id, bos=self._lm.bos_id >= 0, eos=False,
                                                top_n=max(int(cutoff_top_n), 0), closed=lexicon == "closed")
                self._uploaded = False
                return
            tok = self._lm.label_tokens(self.labels)
            if not any(t >= 0 for v, t in enumerate(tok) if v != blank_id):
                raise ValueError("no non-blank label is a token of the model (a word-level LM?): decode without "
                                 "model_path and re-rank with CTCDecoder.lm_rescore(..., "
                                 "lm.label_mapper(labels, mode=\"word\"))")
            self._fused = CTCLMDecoder(len(self.labels), beam_width, self._lm, tok, alpha, beta, blank_id,
                                       bos=self._lm.bos_id >= 0, eos=False, top_n=max(int(cutoff_top_n), 0))
            self._uploaded = False
            return
        self._dec = CTCDecoder(len(self.labels), beam_width, blank_id)
        self._dec.set_timesteps(self.track_timesteps)

    def decode(self, probs, seq_lens=None):
        B, T, V = (int(x) for x in probs.shape)
        lens = None if seq_lens is None else np.asarray(
            seq_lens.cpu().numpy() if hasattr(seq_lens, "cpu") else seq_lens, dtype=np.int32)
        dec = self._fused if self._fused is not None else self._dec
        if self._fused is not None and not self._uploaded:
            self._lm.upload()
            if self._lex is not None:
                self._lex.upload()
            self._uploaded = True
        if hasattr(probs, "is_cuda") and probs.is_cuda:   # torch GPU tensor: zero-copy
            import torch
            p = probs if probs.dtype == torch.float32 else probs.float()
            if p.stride(2) != 1:   # the kernel reads a frame's V labels contiguously
                p = p.contiguous()
            dec.decode_device(p.data_ptr(), T, B, self.log_probs_input,
                              torch.cuda.current_stream().cuda_stream, lens,
                              p.stride(1), p.stride(0))
        else:
            arr = probs.cpu().numpy() if hasattr(probs, "cpu") else np.asarray(probs)
            dec.decode(arr, is_log=self.log_probs_input, lengths=lens, batch_major=True)
        K = self.beam_width
        if self._fused is not None:
            beams = [[(lab, total, None) for lab, total, _, _, _ in u] for u in self._fused.beams(256)]
        elif self.track_timesteps:
            beams = self._dec.beams_ts(max_hyps=self._dec.config()[0])
        else:
            beams = [[(lab, lp, None) for lab, lp in u] for u in self._dec.beams(self._dec.config()[0])]
        results = np.zeros((B, K, T), np.int32)
        scores = np.full((B, K), np.inf, np.float32)
        timesteps = np.full((B, K, T), -1, np.int32)
        out_lens = np.zeros((B, K), np.int32)
        for b, hyps in enumerate(beams):
            for k, (lab, lp, ts) in enumerate(hyps[:K]):
                results[b, k, :len(lab)] = lab
                scores[b, k] = -lp
                if ts is not None:
                    timesteps[b, k, :len(ts)] = ts
                out_lens[b, k] = len(lab)
        return results, scores, timesteps, out_lens
