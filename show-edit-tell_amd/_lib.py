"""ctypes binding of the C-ABI library csrc/libset_hip.so (include/set_hip.h).

The product path has no CPU fallback: if the library is missing or a call fails this module
raises.  PyTorch is used only for device memory and streams; every tensor crosses the boundary
as a raw device pointer + sizes.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SET_LIB_VARIANT=exp: the experimental build of the same sources (build.py LIB_EXP; bench.py's `experimental` leg and the
# split-precision parity test run in child processes with it).  Anything else: the shipped library.
LIB_PATH = os.path.join(_HERE, "csrc", "libset_hip_exp.so" if os.environ.get("SET_LIB_VARIANT") == "exp" else "libset_hip.so")

SET_OK = 0
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3

c_f32p = C.c_void_p
c_i64p = C.c_void_p


class SetError(RuntimeError):
    pass


class EditNetDims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "T", "R", "F", "D", "A", "V", "maxT", "adaptive")]


EDITNET_WEIGHT_FIELDS = (
    # (struct field, state_dict key)
    ("embed", "embed.embedding.weight"),
    ("enc_x2h_w", "caption_encoder.lstm_encoder_cell.x2h.weight"),
    ("enc_x2h_b", "caption_encoder.lstm_encoder_cell.x2h.bias"),
    ("enc_h2h_w", "caption_encoder.lstm_encoder_cell.h2h.weight"),
    ("enc_h2h_b", "caption_encoder.lstm_encoder_cell.h2h.bias"),
    ("enc_aff_w", "caption_encoder.affine_hn.weight"),
    ("enc_aff_b", "caption_encoder.affine_hn.bias"),
    ("ca_feat_w", "caption_attention.cap_features_att.weight"),
    ("ca_feat_b", "caption_attention.cap_features_att.bias"),
    ("ca_dec_w", "caption_attention.cap_decoder_att.weight"),
    ("ca_dec_b", "caption_attention.cap_decoder_att.bias"),
    ("ca_full_w", "caption_attention.cap_full_att.weight"),
    ("ca_full_b", "caption_attention.cap_full_att.bias"),
    ("ca_gate_w", "caption_attention.context_gate.weight"),
    ("ca_gate_b", "caption_attention.context_gate.bias"),
    ("ca_sc_w", "caption_attention.sc_affine.weight"),
    ("ca_sc_b", "caption_attention.sc_affine.bias"),
    ("ca_tc_w", "caption_attention.tc_affine.weight"),
    ("ca_tc_b", "caption_attention.tc_affine.bias"),
    ("va_emb_w", "visual_attention.att_embed.0.weight"),
    ("va_emb_b", "visual_attention.att_embed.0.bias"),
    ("va_feat_w", "visual_attention.features_att.weight"),
    ("va_feat_b", "visual_attention.features_att.bias"),
    ("va_dec_w", "visual_attention.decoder_att.weight"),
    ("va_dec_b", "visual_attention.decoder_att.bias"),
    ("va_full_w", "visual_attention.full_att.weight"),
    ("va_full_b", "visual_attention.full_att.bias"),
    ("al_wih", "attention_lstm.weight_ih"),
    ("al_whh", "attention_lstm.weight_hh"),
    ("al_bih", "attention_lstm.bias_ih"),
    ("al_bhh", "attention_lstm.bias_hh"),
    ("cl_x2h_w", "copy_lstm.x2h.weight"),
    ("cl_x2h_b", "copy_lstm.x2h.bias"),
    ("cl_h2h_w", "copy_lstm.h2h.weight"),
    ("cl_h2h_b", "copy_lstm.h2h.bias"),
    ("cl_cnew_w", "copy_lstm.gate_cnew.weight"),
    ("cl_cnew_b", "copy_lstm.gate_cnew.bias"),
    ("cl_cmem_w", "copy_lstm.gate_cmem.weight"),
    ("cl_cmem_b", "copy_lstm.gate_cmem.bias"),
    ("fc_w", "fc.weight"),
    ("fc_b", "fc.bias"),
)


class EditNetWeights(C.Structure):
    # the state_dict tensors + the optional derived token table (include/set_hip.h)
    _fields_ = [(f, C.c_void_p) for f, _ in EDITNET_WEIGHT_FIELDS] + [("tok_table", C.c_void_p)]


class EditTrace(C.Structure):
    """include/set_hip.h SetEditTrace: output pointers of set_editnet_edit_trace (gate_full / alpha_v may be NULL)"""
    _fields_ = [(n, C.c_void_p) for n in ("alpha_c", "select", "copy_gate", "gate_full", "alpha_v", "logp")]


class ProfileEntry(C.Structure):
    _fields_ = [("tag", C.c_char * 32), ("launches", C.c_int), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


def profile_report(max_entries=64):
    """[{tag, launches, ms, flops, bytes}] aggregated since set_profile_enable(1)."""
    lib = load()
    arr = (ProfileEntry * max_entries)()
    n = lib.set_profile_report(arr, max_entries)
    if n < 0:
        check(-n, "set_profile_report")
    return [dict(tag=arr[i].tag.decode(), launches=arr[i].launches, ms=arr[i].ms, flops=arr[i].flops,
                 bytes=arr[i].bytes) for i in range(n)]


class DcnetDims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "T", "D", "A", "C", "E", "V", "maxT")]


DCNET_WEIGHT_FIELDS = (
    ("embed", "embed.embedding.weight"),
    ("enc_wih_f", "caption_encoder.lstm_encoder.weight_ih_l0"),
    ("enc_whh_f", "caption_encoder.lstm_encoder.weight_hh_l0"),
    ("enc_bih_f", "caption_encoder.lstm_encoder.bias_ih_l0"),
    ("enc_bhh_f", "caption_encoder.lstm_encoder.bias_hh_l0"),
    ("enc_wih_b", "caption_encoder.lstm_encoder.weight_ih_l0_reverse"),
    ("enc_whh_b", "caption_encoder.lstm_encoder.weight_hh_l0_reverse"),
    ("enc_bih_b", "caption_encoder.lstm_encoder.bias_ih_l0_reverse"),
    ("enc_bhh_b", "caption_encoder.lstm_encoder.bias_hh_l0_reverse"),
    ("enc_cat_w", "caption_encoder.concat.weight"),
    ("enc_cat_b", "caption_encoder.concat.bias"),
    ("ca_feat_w", "caption_attention.cap_features_att.weight"),
    ("ca_feat_b", "caption_attention.cap_features_att.bias"),
    ("ca_dec_w", "caption_attention.cap_decoder_att.weight"),
    ("ca_dec_b", "caption_attention.cap_decoder_att.bias"),
    ("ca_full_w", "caption_attention.cap_full_att.weight"),
    ("ca_full_b", "caption_attention.cap_full_att.bias"),
    ("al_wih", "attention_lstm.weight_ih"),
    ("al_whh", "attention_lstm.weight_hh"),
    ("al_bih", "attention_lstm.bias_ih"),
    ("al_bhh", "attention_lstm.bias_hh"),
    ("ll_wih", "language_lstm.weight_ih"),
    ("ll_whh", "language_lstm.weight_hh"),
    ("ll_bih", "language_lstm.bias_ih"),
    ("ll_bhh", "language_lstm.bias_hh"),
    ("fc_w", "fc.weight"),
    ("fc_b", "fc.bias"),
)


class DcnetWeights(C.Structure):
    _fields_ = [(f, C.c_void_p) for f, _ in DCNET_WEIGHT_FIELDS] + [("tok_table", C.c_void_p)]


class GemmDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_longlong), ("B", C.c_void_p), ("ldb", C.c_longlong),
                ("C", C.c_void_p), ("ldc", C.c_longlong), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("accumulate", C.c_int)]


class GemmNtSeg(C.Structure):
    """include/set_hip.h SetGemmNtSeg: one (A, W) column segment of a grouped NT GEMM problem"""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("W", C.c_void_p), ("ldw", C.c_int64), ("K", C.c_int32),
                ("pad_", C.c_int32)]


class GemmNtProb(C.Structure):
    """include/set_hip.h SetGemmNtProb"""
    _fields_ = [("seg", GemmNtSeg * 3), ("C", C.c_void_p), ("ldc", C.c_int64), ("bias", C.c_void_p), ("nseg", C.c_int32),
                ("M", C.c_int32), ("N", C.c_int32), ("act", C.c_int32), ("ksplit", C.c_int32), ("pad_", C.c_int32)]


class GemmNtLaunch(C.Structure):
    """include/set_hip.h SetGemmNtLaunch (ksplit_out / rows_out are HOST pointers)"""
    _fields_ = [("row_list", C.c_void_p), ("row_count", C.c_void_p), ("alive", C.c_void_p), ("ksplit_out", C.c_void_p),
                ("rows_out", C.c_void_p), ("bm_hint", C.c_int32), ("flags", C.c_int32)]


GEMM_NT_NO_ASM, GEMM_NT_KEEP_SLABS = 1, 2


class PickTail(C.Structure):
    """include/set_hip.h SetPickTail: the LSTM-cell tail of the pick kernels"""
    _fields_ = [("g0", C.c_void_p), ("g0_stride", C.c_int64), ("g0_ld", C.c_int64), ("pre", C.c_void_p), ("ldpre", C.c_int64),
                ("tab", C.c_void_p), ("ld_tab", C.c_int64), ("c_in", C.c_void_p), ("c_out", C.c_void_p), ("h_out", C.c_void_p),
                ("g0_n", C.c_int32), ("col0", C.c_int32), ("nrows", C.c_int32), ("D", C.c_int32)]


class PickArgs(C.Structure):
    """include/set_hip.h SetPickArgs (set_pick_slabs_f32)"""
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("stride", C.c_int64), ("bias", C.c_void_p), ("end_idx", C.c_int64),
                ("seq", C.c_void_p), ("seq_logp", C.c_void_p), ("it", C.c_void_p), ("unfinished", C.c_void_p),
                ("alive", C.c_void_p), ("table", C.c_void_p), ("emb_out", C.c_void_p), ("seed", C.c_uint64),
                ("offset", C.c_uint64), ("raw_ids", C.c_void_p), ("lse", C.c_void_p), ("step_logp", C.c_void_p),
                ("tail", C.POINTER(PickTail)), ("n", C.c_int32), ("B", C.c_int32), ("V", C.c_int32), ("t", C.c_int32),
                ("max_len", C.c_int32), ("D", C.c_int32), ("mode", C.c_int32), ("pad_", C.c_int32)]


PICK_GREEDY, PICK_SAMPLE = 0, 1


class SbsArgs(C.Structure):
    """include/set_hip.h SetSbsArgs (set_sbs_pick_f32: the stochastic beam search pick)"""
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("end_idx", C.c_int64), ("seed", C.c_uint64), ("offset", C.c_uint64),
                ("phi", C.c_void_p), ("G", C.c_void_p), ("finished", C.c_void_p), ("len", C.c_void_p), ("seqs_in", C.c_void_p),
                ("seqs_out", C.c_void_p), ("words", C.c_void_p), ("rows", C.c_void_p), ("n_open", C.c_void_p), ("ws", C.c_void_p),
                ("ws_bytes", C.c_size_t), ("NI", C.c_int32), ("k", C.c_int32), ("V", C.c_int32), ("t", C.c_int32),
                ("Lmax", C.c_int32), ("pad_", C.c_int32)]


class BeamConstraintsC(C.Structure):
    """include/set_hip.h SetBeamConstraints (set_beam_pick_constrained_f32; the user-facing object: evaluate.BeamConstraints)"""
    _fields_ = [("no_repeat_ngram", C.c_int32), ("min_len", C.c_int32), ("length_alpha", C.c_float), ("n_banned", C.c_int32),
                ("banned", C.c_void_p)]


class SampleOpts(C.Structure):
    """include/set_hip.h SetSampleOpts: temperature, top-k and top-p of the sampled pick ({1, 0, 1}: neutral)"""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("pad_", C.c_int32)]


def sample_opts(temperature=1.0, top_k=0, top_p=1.0):
    """None for neutral values (the caller then makes the call without options), a checked SampleOpts otherwise"""
    import math
    if float(temperature) == 1.0 and int(top_k) == 0 and float(top_p) == 1.0:
        return None
    t, p = float(temperature), float(top_p)
    if not (math.isfinite(t) and 1e-3 <= t <= 1e3):
        raise ValueError("temperature must be a finite number in [1e-3, 1e3], got %r" % (temperature,))
    if int(top_k) != top_k or top_k < 0:
        raise ValueError("top_k must be an integer >= 0 (0: off), got %r" % (top_k,))
    if not (math.isfinite(p) and 0.0 < p <= 1.0):
        raise ValueError("top_p must lie in (0, 1] (1: off), got %r" % (top_p,))
    return SampleOpts(temperature=t, top_k=int(top_k), top_p=p)


SAMPLERS = ("cdf", "gumbel")


def check_sampler_name(sampler, top_k, top_p):
    """the part of check_sampler that needs no tensor: made first, so that a wrong option is a ValueError wherever the inputs live"""
    if sampler not in SAMPLERS:
        raise ValueError("sampler must be one of %r, got %r" % (SAMPLERS, sampler))
    if sampler == "gumbel" and (int(top_k) != 0 or float(top_p) != 1.0):
        raise ValueError('sampler="gumbel" takes the temperature only: top_k / top_p truncation needs sampler="cdf"')


def check_sampler(sampler, opts, sample_max, sample_rl, grad_path):
    """sampler="cdf" (default: the inverse-CDF draw) | "gumbel" (the Gumbel-max draw, include/set_hip.h): "gumbel" takes the
    temperature only and exists on the no-grad sampled rollout only.  Returns True for "gumbel"."""
    if sampler == "cdf":
        return False
    check_sampler_name(sampler, 0 if opts is None else opts.top_k, 1.0 if opts is None else opts.top_p)
    if sample_max or not sample_rl:
        raise ValueError('sampler="gumbel" applies to the sampled rollout only (sample_max=False, sample_rl=True)')
    if grad_path:
        raise ValueError('sampler="gumbel" is not supported in the grad-enabled rollout (train mode or parameters that require '
                         "grad): call the model in eval mode under torch.no_grad()")
    return True


def refuse_sample_opts(sample_max, sample_rl, grad_path):
    """non-neutral sampling options where nothing is sampled, or where the log-probs would need a backward that is not built"""
    if sample_max or not sample_rl:
        raise ValueError("temperature / top_k / top_p apply to the sampled rollout only (sample_max=False, sample_rl=True)")
    if grad_path:
        raise ValueError("temperature / top_k / top_p are not supported in the grad-enabled rollout (train mode or parameters "
                         "that require grad): call the model in eval mode under torch.no_grad()")


def decode_constraints(constraints, word_map, V, sample_max, sample_rl, grad_path, gumbel):
    """`constraints=` of the free-running decodes (editnet_rl.DecoderC.forward, dcnet_rl.DAE.forward): None for None and for a
    neutral evaluate.BeamConstraints (the caller then makes exactly today's calls), otherwise the checked object and its banned
    ids — resolved once against the vocabulary, before any device work.  ValueError: a length penalty (nothing is ranked in
    these decodes), sampler="gumbel", and every path in which gradients flow (no backward of the constrained pick is built)."""
    from . import evaluate
    cons = evaluate._active(constraints)
    if cons is None:
        return None
    ids = cons.banned_ids(word_map, V)
    if cons.length_penalty != 0.0:
        raise ValueError("constraints.length_penalty applies to beam search only (greedy and sampled decodes rank nothing)")
    if gumbel:
        raise ValueError('constraints are not built into sampler="gumbel": use sampler="cdf"')
    if grad_path:
        raise ValueError("constraints are not supported in the grad-enabled rollout (train mode or parameters that require "
                         "grad): call the model in eval mode under torch.no_grad()")
    if not sample_max and not sample_rl:
        raise ValueError("constraints apply to the greedy (sample_max=True) and the sampled (sample_rl=True) decode")
    return cons, ids


def refuse_constraints(constraints, where):
    """the entries through which gradients flow (sample_rollout, the SCST steps): an active `constraints=` is a ValueError there"""
    from . import evaluate
    if evaluate._active(constraints) is not None:
        raise ValueError("constraints are not supported in %s: no backward of the constrained pick is built (decode in eval "
                         "mode under torch.no_grad())" % where)


def constraints_struct(cons_ids, device):
    """(BeamConstraintsC, the device tensor of banned ids it points to — keep it alive over the call) of decode_constraints' answer"""
    import torch
    cons, ids = cons_ids
    banned = torch.tensor(ids, dtype=torch.long, device=device) if ids else None
    return BeamConstraintsC(cons.no_repeat_ngram, cons.min_length, 0.0, len(ids), banned.data_ptr() if ids else None), banned


class SlabSrc(C.Structure):
    """include/set_hip.h SetSlabSrc: one addend of a gradient that is still split-K partials"""
    _fields_ = [("p", C.c_void_p), ("slab_stride", C.c_int64), ("ld", C.c_int64), ("nslab", C.c_int32), ("rows", C.c_int32)]


class ColsumDesc(C.Structure):
    """include/set_hip.h SetColsumDesc: one column sum of a grouped launch (set_colsum_group_f32)"""
    _fields_ = [("x", C.c_void_p), ("ld", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("out", C.c_void_p),
                ("accumulate", C.c_int32), ("out2", C.c_void_p), ("accumulate2", C.c_int32)]


def _fields(spec):
    """'int a, b; float c; ptr d, e' style field list -> ctypes _fields_"""
    kinds = {"int": C.c_int, "float": C.c_float, "u64": C.c_uint64, "i64": C.c_int64, "ptr": C.c_void_p, "size": C.c_size_t}
    out = []
    for part in spec.split(";"):
        part = part.strip()
        if not part:
            continue
        kind, names = part.split(None, 1)
        for nme in names.split(","):
            nme = nme.strip()
            if "[" in nme:
                base, cnt = nme[:-1].split("[")
                out.append((base, kinds[kind] * int(cnt)))
            else:
                out.append((nme, kinds[kind]))
    return out


class XELoopArgs(C.Structure):
    """include/set_hip.h SetXELoopArgs"""
    _fields_ = _fields("int T, B, R, F, Tc, D, A, V, train; float p_embed, p_out; u64 seed, off_embed, off_out; ptr bts; ptr w; "
                       "ptr E, al_wih, al_whh; ptr tok; i64 tok_step, tok_stride; ptr X, H, Mem, mask, att1_c, pre1, att1; "
                       "i64 att1_step; ptr EMB, H1, C1, H2, C2, G1, G2, WHC, ZT, S, TT, ALPHAC, ALPHAV, ATT2C, ATT2V, SEL, CNEW, CG, "
                       "X2, H2D; ptr gated, cx, aimg; ptr ws_l; size ws_l_bytes; ptr ws_c; size ws_c_bytes; ptr ws_k; size ws_k_bytes; "
                       "int step_logs; ptr rmask; i64 rmask_step")


class XEBwdLoopArgs(C.Structure):
    """include/set_hip.h SetXEBwdLoopArgs"""
    _fields_ = _fields("int T, B, R, F, Tc, D, A, acc_datt1; float p_out; u64 seed, off_out; ptr bts; "
                       "ptr cl_cnew_w, cl_cmem_w, cl_x2h_w, cl_h2h_w, w_ctx, w_h1, dec_cat, al_wih, al_whh, va_full, ca_full; "
                       "ptr G1, G2, C1, C2, CG, SEL, CNEW, ZT, S, TT, ALPHAC, ALPHAV, ATT2C, ATT2V, X, H, Mem, att1_c, att1; "
                       "i64 att1_step; ptr dH2D; ptr DU, DGW, DSZT, DATT2, DWFC, DWFV, DEC, DEV, DCTX, DG1, datt1; i64 datt1_step; "
                       "ptr datt1c, dMem; ptr DC1[2], DC2[2]; ptr dcm, dcn, dop, dalc; ptr slab_ws[5]; size slab_ws_bytes; ptr tmp[11]; "
                       "ptr DLAST")


_P = C.c_void_p
_I = C.c_int
_L = C.c_int64
_Z = C.c_size_t
_U = C.c_uint64

# name -> (restype, argtypes); mirrors include/set_hip.h one to one
PROTOTYPES = {
    "set_abi_version": (_I, []),
    "set_error_string": (C.c_char_p, [_I]),
    "set_last_hip_error": (_I, []),
    "set_last_hip_error_string": (C.c_char_p, []),
    "set_target_arch": (C.c_char_p, []),
    "set_profile_enable": (_I, [_I]),
    "set_profile_report": (_I, [_P, _I]),
    "set_editnet_workspace_bytes": (_Z, [C.POINTER(EditNetDims)]),
    "set_editnet_token_table_bytes": (_Z, [C.POINTER(EditNetDims)]),
    "set_editnet_token_table_workspace_bytes": (_Z, [C.POINTER(EditNetDims)]),
    "set_editnet_build_token_table": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _Z, _P]),
    "set_editnet_begin": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _P, _Z, _P]),
    "set_editnet_begin_greedy": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _P, _Z, _P]),
    "set_editnet_step": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _L, _I, _P, _L, _P, _Z, _P]),
    "set_editnet_greedy_pick": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _L, _I, _L, _P, _P, _I,
                                     _P, _Z, _P]),
    "set_editnet_greedy": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _P, _P,
                                _P, _Z, _P]),
    "set_decode_row_limits": (_I, [_P]),
    "set_editnet_greedy_begun": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _L, _L, _I, _P, _P, _P, _Z, _P]),
    "set_editnet_beam_persistent": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _P, _P, _P, _P, _P,
                                         _P, _Z, _P]),
    "set_editnet_beam_persistent_nbest": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _P, _P, _P,
                                               _P, _P, _P, _Z, _P, _P]),
    "set_editnet_sample": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _U, _U, _P,
                                _P, _P, _Z, _P]),
    "set_editnet_sample_opts": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _U, _U, _P,
                                     _P, _P, _Z, _P, C.POINTER(SampleOpts)]),
    "set_editnet_sample_gumbel": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _U, _U, _P,
                                       _P, _P, _Z, _P, C.POINTER(SampleOpts)]),
    "set_editnet_gumbel_persistent": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _U, _U, _P,
                                           _P, _P, _Z, _P, C.POINTER(SampleOpts)]),
    "set_editnet_xe_forward": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _L,
                                    C.POINTER(C.c_int), _P, _P, _P, _P, _Z, _P]),
    "set_editnet_edit_trace_workspace_bytes": (_Z, [C.POINTER(EditNetDims), _I]),
    "set_editnet_edit_trace": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _P, _L, _P, _I,
                                    C.POINTER(EditTrace), _P, _Z, _P, _Z, _P]),
    "set_editnet_ws_tensor": (_P, [C.POINTER(EditNetDims), _P, C.c_char_p]),
    "set_dcnet_workspace_bytes": (_Z, [C.POINTER(DcnetDims)]),
    "set_dcnet_token_table_bytes": (_Z, [C.POINTER(DcnetDims)]),
    "set_dcnet_token_table_workspace_bytes": (_Z, [C.POINTER(DcnetDims)]),
    "set_dcnet_build_token_table": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _Z, _P]),
    "set_dcnet_begin": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _P, _Z, _P]),
    "set_dcnet_step": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _L, _I, _P, _L, _P, _Z, _P]),
    "set_dcnet_greedy_pick": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _L, _I, _L, _P, _P, _I, _P, _Z,
                                   _P]),
    "set_dcnet_greedy": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _P, _P, _P, _Z, _P]),
    "set_dcnet_beam_persistent": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _P, _P, _P, _P, _P, _P, _Z,
                                       _P]),
    "set_dcnet_beam_persistent_nbest": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _P, _P, _P, _P, _P, _P,
                                             _Z, _P, _P]),
    "set_ensemble_beam_persistent": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), C.POINTER(DcnetWeights), C.POINTER(DcnetDims),
                                          _P, _P, _P, _L, _L, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _P, _Z, _P]),
    "set_ensemble_beam_persistent_nbest": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), C.POINTER(DcnetWeights),
                                                C.POINTER(DcnetDims), _P, _P, _P, _L, _L, _I, _P, _P, _P, _P, _P, _P, _Z, _P, _Z, _P, _Z,
                                                _P, _P]),
    "set_ensemble_beam_xbuf_bytes": (_Z, [C.POINTER(EditNetDims), C.POINTER(DcnetDims)]),
    "set_dcnet_sample": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _U, _U, _P, _P, _P, _Z,
                              _P]),
    "set_dcnet_sample_opts": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _U, _U, _P, _P, _P, _Z,
                                   _P, C.POINTER(SampleOpts)]),
    "set_dcnet_sample_gumbel": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _U, _U, _P, _P, _P, _Z,
                                     _P, C.POINTER(SampleOpts)]),
    "set_dcnet_gumbel_persistent": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _U, _U, _P, _P, _P, _Z,
                                         _P, C.POINTER(SampleOpts)]),
    "set_dcnet_xe_forward": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _L, C.POINTER(C.c_int), _P, _P,
                                  _P, _P, _Z, _P]),
    "set_dcnet_xe_forward_hidden": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _L, C.POINTER(C.c_int), _P,
                                         _P, _P, _P, _P, _Z, _P]),
    "set_dcnet_ws_tensor": (_P, [C.POINTER(DcnetDims), _P, C.c_char_p]),
    "set_linear_workspace_bytes": (_Z, [_I, _I, _I]),
    "set_linear_f32": (_I, [_P, _L, _P, _L, _P, _P, _L, _I, _I, _I, _I, _P, _Z, _P]),
    "set_gemm_nt_group_workspace_bytes": (_Z, [C.POINTER(GemmNtProb), _I]),
    "set_gemm_nt_group_f32": (_I, [C.POINTER(GemmNtProb), _I, C.POINTER(GemmNtLaunch), _P, _Z, _P]),
    "set_gemm_nt_greedy_scope": (_I, [_I]),
    "set_embed_relu_f32": (_I, [_P, _P, _L, _P, _L, _I, _I, _I, _P]),
    "set_lstm_cell_workspace_bytes": (_Z, [_I, _I, _I]),
    "set_lstm_cell_f32": (_I, [_P, _L, _I, _P, _P, _P, _L, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "set_caption_attention_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "set_caption_attention_f32": (_I, [C.POINTER(EditNetWeights), _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P,
                                       _Z, _P]),
    "set_visual_attention_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "set_visual_attention_f32": (_I, [C.POINTER(EditNetWeights), _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _Z,
                                      _P]),
    "set_visual_attention_masked_f32": (_I, [C.POINTER(EditNetWeights), _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P,
                                             _Z, _P]),
    "set_select_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "set_select_soft_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "set_select_soft_bwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "set_copy_lstm_workspace_bytes": (_Z, [_I, _I, _I]),
    "set_copy_lstm_f32": (_I, [C.POINTER(EditNetWeights), _P, _L, _I, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "set_lstm_cell_train_f32": (_I, [_P, _L, _I, _P, _P, _P, _L, _P, _P, _P, _P, _P, _P, _I, _I, _P, _Z, _P]),
    "set_lstm_cell_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "set_copy_lstm_train_f32": (_I, [C.POINTER(EditNetWeights), _P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P,
                                     _Z, _P]),
    "set_copy_gate_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "set_lstm_gates_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "set_caption_attention_train_f32": (_I, [C.POINTER(EditNetWeights), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I,
                                             _I, _I, _I, _I, _P, _Z, _P]),
    "set_context_gate_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "set_attention_bwd_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "set_encoder_cell_workspace_bytes": (_Z, [_I, _I]),
    "set_encoder_cell_train_f32": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _P,
                                        _Z, _P]),
    "set_encoder_cell_bwd_f32": (_I, [_P, _P, _P, _P, _L, _L, _I, _P, _I, _P, _P, _P, _P, _L, _P, _P, _I, _I, _P]),
    "set_select_bwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "set_editnet_attentions_workspace_bytes": (_Z, [_I, _I, _I]),
    "set_editnet_attentions_train_f32": (_I, [C.POINTER(EditNetWeights)] + [_P] * 20 + [_I] * 6 + [_P, _Z, _P]),
    "set_copy_gate_bwd_ld_f32": (_I, [_P, _P, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "set_caption_attention_att2_f32": (_I, [C.POINTER(EditNetWeights), _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P,
                                            _Z, _P]),
    "set_context_gate_bwd_ld_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    "set_lstm_cell_pre_train_f32": (_I, [_P, _L, _P, _L, _I, _P, _L, _P, _L, _I, _P, _P, _P, _L, _P, _P, _P, _P, _I, _I, _P, _Z,
                                         _P]),
    "set_select_bwd_acc_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "set_attention_bwd_acc_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _P]),
    "set_attention_dvalues_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "set_xe_loss_f32": (_I, [_P, _L, _L, _P, _L, _L, _P, _I, _I, _I, _P, _P, _P, _P]),
    "set_xe_loss_bwd_f32": (_I, [_P, _L, _L, _P, _L, _L, _P, _I, _I, _I, _P, _P, _P, _L, _P]),
    "set_mse_sum_f32": (_I, [_P, _P, _L, _P, _P]),
    "set_mse_bwd_f32": (_I, [_P, _P, _L, C.c_float, _P, _P, _P, _P]),
    "set_clip_adam_workspace_bytes": (_Z, [_I, _P]),
    "set_clip_adam_f32": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, _I, _P, _P, _Z, _P]),
    "set_colsum_workspace_bytes": (_Z, [_I]),
    "set_colsum_f32": (_I, [_P, _L, _I, _I, _P, _I, _P, _Z, _P]),
    "set_colsum_group_workspace_bytes": (_Z, [_P, _I]),
    "set_colsum_group_f32": (_I, [_P, _I, _P, _Z, _P]),
    "set_dropout_f32": (_I, [_P, _L, _P, _L, _I, _I, C.c_float, _U, _U, _P]),
    "set_embed_relu_dropout_f32": (_I, [_P, _P, _L, _P, _L, _I, _I, _I, C.c_float, _U, _U, _P]),
    "set_dropout_bwd_f32": (_I, [_P, _L, _P, _L, _P, _L, _I, _I, C.c_float, _I, _P]),
    "set_dropout_steps_f32": (_I, [_P, _L, _P, _L, _L, _I, _I, _I, C.c_float, _U, _U, _P]),
    "set_dropout_bwd_steps_f32": (_I, [_P, _L, _L, _P, _L, _L, _P, _L, _I, _I, _I, C.c_float, _I, _P]),
    "set_dropout_bwd_philox_f32": (_I, [_P, _L, _P, _L, _I, _I, C.c_float, _U, _U, _I, _P]),
    "set_rowsum_mask_f32": (_I, [_P, _L, _I, _I, _P, _P]),
    "set_pack_f32": (_I, [_P, _L, _I, _I, C.POINTER(_P), C.POINTER(_L), C.POINTER(_I), _I, _P]),
    "set_sample_pick_f32": (_I, [_P, _L, _I, _I, _I, _I, _L, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P]),
    "set_sample_pick_opts_f32": (_I, [_P, _L, _I, _I, _I, _I, _L, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(SampleOpts)]),
    "set_sample_pick_opts_key_f32": (_I, [_P, _L, _I, _I, _I, _I, _L, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(SampleOpts), _P]),
    "set_sample_logp_bwd_f32": (_I, [_P, _L, _P, _P, _P, _P, _L, _I, _I, _P]),
    "set_sample_logp_bwd_opts_f32": (_I, [_P, _L, _P, _P, _P, _P, _P, _L, _I, _I, C.POINTER(SampleOpts), _P]),
    "set_philox4x32": (_I, [_P, _I, _U, _U, _P]),
    "set_gumbel_pick_f32": (_I, [_P, _L, _I, _I, _I, _I, _L, _U, _U, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(SampleOpts)]),
    "set_gumbel_fill_f32": (_I, [_P, _I, _I, _I, _U, _U, _P]),
    "set_pick_slabs_f32": (_I, [C.POINTER(PickArgs), _P]),
    "set_pick_slabs_opts_f32": (_I, [C.POINTER(PickArgs), C.POINTER(SampleOpts), _P]),
    "set_pick_slabs_constrained_f32": (_I, [C.POINTER(PickArgs), C.POINTER(SampleOpts), C.POINTER(BeamConstraintsC), _P]),
    "set_editnet_greedy_constrained": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _P, _P,
                                            _P, _Z, _P, C.POINTER(BeamConstraintsC)]),
    "set_editnet_sample_constrained": (_I, [C.POINTER(EditNetWeights), C.POINTER(EditNetDims), _P, _P, _P, _P, _L, _L, _I, _U, _U,
                                            _P, _P, _P, _Z, _P, C.POINTER(SampleOpts), C.POINTER(BeamConstraintsC)]),
    "set_dcnet_greedy_constrained": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _P, _P, _P, _Z, _P,
                                          C.POINTER(BeamConstraintsC)]),
    "set_dcnet_sample_constrained": (_I, [C.POINTER(DcnetWeights), C.POINTER(DcnetDims), _P, _P, _L, _L, _I, _U, _U, _P, _P, _P, _Z,
                                          _P, C.POINTER(SampleOpts), C.POINTER(BeamConstraintsC)]),
    "set_beam_pick_f32": (_I, [_P, _P, _L, _I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "set_beam_pick_nbest_f32": (_I, [_P, _P, _L, _I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "set_beam_gather_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "set_beam_pick_constrained_workspace_bytes": (_Z, [_I, _I]),
    "set_beam_pick_constrained_f32": (_I, [_P, _P, _L, _I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                           C.POINTER(BeamConstraintsC), _P, _Z, _P]),
    "set_beam_pick_diverse_workspace_bytes": (_Z, [_I, _I]),
    "set_beam_pick_diverse_f32": (_I, [_P, _P, _L, _I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                       _P, _P, _I, C.c_float, C.POINTER(BeamConstraintsC), _P, _Z, _P]),
    "set_sbs_workspace_bytes": (_Z, [_I, _I]),
    "set_sbs_pick_f32": (_I, [C.POINTER(SbsArgs), C.POINTER(SampleOpts), _P]),
    "set_sbs_pick_ensemble_f32": (_I, [C.POINTER(SbsArgs), _P, C.POINTER(SampleOpts), _P]),
    "set_sbs_pick_opts_f32": (_I, [C.POINTER(SbsArgs), C.POINTER(SampleOpts), _P]),
    "set_sbs_pick_ensemble_opts_f32": (_I, [C.POINTER(SbsArgs), _P, C.POINTER(SampleOpts), _P]),
    "set_gemm_group_f32": (_I, [C.POINTER(GemmDesc), _I, _I, _I, _P, _Z, _P]),
    "set_gemm_group_slabs_f32": (_I, [C.POINTER(GemmDesc), _I, _I, _I, _P, _Z, C.POINTER(SlabSrc), _P]),
    "set_editnet_xe_train_loop_f32": (_I, [C.POINTER(XELoopArgs), _P]),
    "set_editnet_xe_train_bwd_loop_f32": (_I, [C.POINTER(XEBwdLoopArgs), _P]),
    "set_lstm_cell_bwd_src_f32": (_I, [C.POINTER(SlabSrc), _I, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "set_copy_gate_bwd_src_f32": (_I, [C.POINTER(SlabSrc), _I, _P, _L, C.c_float, _U, _U, _P, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P,
                                       _I, _I, _P]),
    "set_lstm_gates_bwd_src_f32": (_I, [_P, C.POINTER(SlabSrc), _I, _P, _P, _P, _P, _P, _I, _I, _P]),
    "set_select_bwd_src_f32": (_I, [_P, C.POINTER(SlabSrc), _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "set_context_gate_bwd_src_f32": (_I, [_P, C.POINTER(SlabSrc), _I, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P]),
    "set_attention_bwd_src_f32": (_I, [_P, C.POINTER(SlabSrc), _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I,
                                       _L, _P]),
    "set_gemm_f32": (_I, [_P, _L, _I, _P, _L, _I, _P, _L, _I, _I, _I, _I, _P, _Z, _P]),
    "set_ciderd_create": (_P, [_P, _P, _P, _L, C.c_double, _I, C.c_double]),
    "set_ciderd_destroy": (None, [_P]),
    "set_ciderd_score": (_I, [_P, _P, _P, _I, _P, _P, _P, _P, _I, _P]),
    "set_ciderd_device_key": (_I, [_P, _I, _P]),
    "set_ciderd_device_create": (_I, [_P, _P, _P, _L, C.c_double, _I, C.c_double, _P, C.POINTER(_P)]),
    "set_ciderd_device_create_corpus": (_I, [_P, _L, _P, _L, _I, _P, _I, _I, _L, _I, C.c_double, _P, C.POINTER(_P)]),
    "set_ciderd_device_dropped": (_I, [_P, C.POINTER(_L), _P]),
    "set_ciderd_device_destroy": (None, [_P]),
    "set_ciderd_device_lookup": (_I, [_P, _P, _L, _P, _P]),
    "set_ciderd_device_vec_bytes": (_Z, [_I, _I]),
    "set_ciderd_device_vectorise": (_I, [_P, _P, _L, _P, _I, _I, _P, _P]),
    "set_ciderd_device_score": (_I, [_P, _P, _L, _P, _I, _I, _P, _P, _I, _L, _P, _I, _I, _P, _P, _L, _P]),
    "set_bleu_device_ref_bytes": (_Z, [_I, _I]),
    "set_bleu_device_prepare": (_I, [_P, _L, _P, _I, _I, _P, _P]),
    "set_bleu_device_score": (_I, [_P, _L, _P, _I, _I, _P, _P, _I, _L, _P, _I, _I, _P, _P, _P, _L, _P]),
    "set_rouge_device_score": (_I, [_P, _L, _P, _I, _I, _P, _P, _I, _L, _P, _I, _I, C.c_double, _P, _P, _P, _L, _P]),
    "set_edit_device_score": (_I, [_P, _L, _P, _I, _I, _P, _P, _I, _L, _P, _I, _I, _P, _P, _P, _L, _P]),
    "set_edit_device_align": (_I, [_P, _L, _P, _I, _I, _P, _L, _P, _I, _P, _P, _L, _P, _P, _L, _P]),
    "set_caption_encoder_workspace_bytes": (_Z, [_I, _I, _I]),
    "set_caption_encoder_f32": (_I, [C.POINTER(EditNetWeights), _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
}

_lib = None


def load():
    """Load libset_hip.so (once).  Raises SetError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SetError(
            "HIP library %s is missing: build it with `python -m show_edit_tell_amd.build` "
            "(there is no CPU fallback for the decode path)" % LIB_PATH)
    # torch bundles its own HIP runtime (same SONAME as /opt/rocm's): import it FIRST so that this
    # library binds to the runtime that owns torch's device pointers and streams.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            MISSING.append(name)         # header / library drift: calling it raises below; tests assert none
            setattr(lib, name, _missing(name))
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


MISSING = []


def _missing(name):
    def fn(*a, **k):
        raise SetError("libset_hip.so does not export %s (rebuild: python -m show_edit_tell_amd.build --force)" % name)
    return fn


def check(rc: int, what: str = ""):
    if rc == SET_OK:
        return
    lib = load()
    msg = lib.set_error_string(rc).decode()
    if rc == 3:
        msg += ": " + lib.set_last_hip_error_string().decode()
    raise SetError("%s failed (code %d): %s" % (what or "libset_hip call", rc, msg))


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_of(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def pack_weights(struct_cls, fields, params: dict, device):
    """Fill a weights struct from {state_dict key: tensor}; tensors must be fp32, contiguous, on `device`."""
    import torch
    s = struct_cls()
    for f, key in fields:
        t = params[key]
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise SetError("parameter %s must be a contiguous fp32 tensor on %s (got %s, %s, contiguous=%s)"
                           % (key, device, t.dtype, t.device, t.is_contiguous()))
        if t.data_ptr() % 16:
            raise SetError("parameter %s is not 16-byte aligned" % key)
        setattr(s, f, t.data_ptr())
    return s
