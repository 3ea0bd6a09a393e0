"""ctypes binding of libproben_hip.so (include/proben_hip.h).  Fails loudly."""
import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libproben_hip.so")
_lib = None

c_void_p, c_int, c_double, c_float = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_float
c_size_t = ctypes.c_size_t

# name -> argtypes (restype is always int unless listed in _RESTYPE)
SIGNATURES = {
    "pe_version": [],
    "pe_proben_pack_detections": [c_void_p] * 6 + [c_int] * 6 + [c_void_p] * 9,
    "pe_proben_pack_logits": [c_void_p] * 6 + [c_int] * 6 + [c_void_p] * 9,
    "pe_proben_pack_log_posteriors": [c_void_p] * 6 + [c_int] * 6 + [c_void_p] * 10,
    "pe_log_softmax": [c_void_p, ctypes.c_int64, c_int, c_double, c_void_p, c_void_p],
    "pe_calibrated_softmax": [c_void_p, ctypes.c_int64, c_int, c_double, c_void_p, c_void_p],
    "pe_temperature_nll": [c_void_p, c_void_p, ctypes.c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pe_match_ground_truth": [c_void_p] * 6 + [c_int, c_double, c_int] + [c_void_p] * 4,
    "pe_variance_stats": [c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int64, c_void_p, c_double] + [c_void_p] * 4,
    "pe_proben_pack_calibrated": [c_void_p] * 9 + [c_int] * 6 + [c_void_p] * 10,
    "pe_bias_nll": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pe_box_gls_batch": [c_void_p] * 7 + [c_int, c_int, c_void_p, c_int] + [c_void_p] * 3,
    "pe_box_pair_stats": [c_void_p] * 3 + [ctypes.c_int64, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_int64,
                          c_int] + [c_void_p] * 5,
    "pe_proben_pack_pooled": [c_void_p] * 9 + [c_int] * 6 + [c_void_p] * 11,
    "pe_pool_nll": [c_void_p, c_void_p, ctypes.c_int64, c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                    c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "pe_reliability_logits": [c_void_p] * 3 + [ctypes.c_int64, c_int, c_double, c_int] + [c_void_p] * 5,
    "pe_reliability_scores": [c_void_p] * 2 + [ctypes.c_int64, c_int] + [c_void_p] * 5,
    "pe_conv2d_nhwc_f16": [c_void_p] * 5 + [c_int] * 14 + [c_void_p],
    "pe_conv_wd_supported": [c_int] * 6,
    "pe_conv_wd_launch_supported": [c_int] * 6,
    "pe_bneck64_supported": [c_int] * 3,
    "pe_conv_wd_pack_weights": [c_void_p] * 2 + [c_int] * 3 + [c_void_p],
    "pe_conv3x3_wd_f16": [c_void_p] * 4 + [c_int] * 7 + [c_void_p],
    "pe_conv_wd_pack_tail": [c_void_p] * 2 + [c_int] * 2 + [c_void_p],
    "pe_bottleneck_tail_wd_f16": [c_void_p] * 7 + [c_int] * 5 + [c_void_p],
    "pe_bneck64_packed_bytes": [c_int] * 2,
    "pe_bneck64_pack": [c_void_p] * 6,
    "pe_bneck64_f16": [c_void_p] * 9 + [c_int] * 5 + [c_void_p],
    "pe_conv1x1_pair_supported": [c_int] * 3 + [ctypes.c_int64],
    "pe_conv1x1_pair_f16": [c_void_p] * 8 + [c_int] * 6 + [c_void_p],
    "pe_conv_wd_pack_head": [c_void_p] * 2 + [c_int] * 2 + [c_void_p],
    "pe_conv3x3_wd_rpn_head_f16": [c_void_p] * 6 + [c_int] * 4 + [c_void_p],
    "pe_preprocess_pack": [c_void_p] + [c_int] * 11 + [c_void_p] * 4,
    "pe_preprocess_pack_batch": [c_void_p] + [c_int] * 12 + [c_void_p] * 4,
    "pe_preprocess_pack_pil_u8": [c_void_p] + [c_int] * 11 + [c_void_p] * 2 + [c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 2,
    "pe_fusion_input_pack": [c_void_p] * 2 + [c_int] * 12 + [c_void_p] * 4,
    "pe_maxpool3x3s2_nhwc": [c_void_p] * 2 + [c_int] * 4 + [c_void_p],
    "pe_subsample2_nhwc": [c_void_p] * 2 + [c_int] * 4 + [c_void_p],
    "pe_stem_conv7x7_maxpool_f16": [c_void_p] * 4 + [c_int] * 3 + [c_void_p],
    "pe_nms_scratch_bytes": [c_int, c_int],
    "pe_nms_batched": [c_void_p] * 5 + [c_int, c_int, c_float, c_int, c_int] + [c_void_p] * 3 + [c_size_t, c_void_p],
    "pe_rpn_select_topk": [c_void_p] * 4 + [c_int] * 4 + [c_void_p, c_float] + [c_void_p] * 4 + [c_int, c_void_p, c_size_t, c_void_p],
    "pe_rpn_scratch_bytes": [c_void_p, c_int, c_int],
    "pe_box2box_apply_deltas": [c_void_p] * 2 + [c_int] * 2 + [c_void_p, c_float, c_void_p, c_void_p],
    "pe_grid_anchors": [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p],
    "pe_gather_boxes": [c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 3,
    "pe_roi_align_nhwc": [c_void_p] * 3 + [c_int] * 4 + [c_void_p] + [c_int] * 3 + [c_void_p] + [c_int] * 4 + [c_void_p] * 3,
    "pe_roi_align_nhwc_sorted": [c_void_p] * 3 + [c_int] * 4 + [c_void_p] + [c_int] + [c_void_p] + [c_int] * 4 + [c_void_p] * 4,
    "pe_sgd_momentum_f32": [c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_float] * 4 + [c_int, c_void_p],
    "pe_roi_align_backward_nhwc": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "pe_boxhead_candidates": [c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 4 + [c_float, c_float, c_int] + [c_void_p] * 8,
    "pe_cocoeval_bbox": [c_void_p] * 6 + [ctypes.c_int64] + [c_void_p] * 4 + [ctypes.c_int64, c_int, c_int, c_void_p, c_int,
                         c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p],
    "pe_boxhead_finalize": [c_void_p] + [c_int] * 7 + [c_void_p] * 18,
    "pe_boxhead_var_vote": [c_void_p] + [c_int] * 6 + [c_void_p] * 6 + [c_float] + [c_void_p] * 2,
    "pe_cocoeval_bbox_matches": [c_void_p] * 6 + [ctypes.c_int64] + [c_void_p] * 4 + [ctypes.c_int64, c_int, c_int, c_void_p, c_int,
                                 c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int] + [c_void_p] * 5,
    "pe_ap_bootstrap": [c_void_p] * 4 + [ctypes.c_int64] + [c_void_p] * 2 + [c_int] * 5 + [c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 5,
    "pe_wbf_fuse_batch": [c_void_p] * 6 + [c_int] * 3 + [c_void_p, c_int, c_double, c_double] + [c_void_p] * 8,
    "pe_lamr_bootstrap": [c_void_p] * 2 + [ctypes.c_int64] + [c_void_p] * 2 + [c_int] * 2 + [c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 4,
    "pe_pdq_pair_quality": [c_void_p] * 10 + [c_int] * 4 + [ctypes.c_int64, c_int, c_void_p, c_double] + [c_void_p] * 7,
    "pe_pdq_assign": [c_void_p] * 6 + [c_int] * 3 + [ctypes.c_int64, c_void_p],
    "pe_tide_classify": [c_void_p] * 7 + [c_int] * 4 + [c_double] * 2 + [c_void_p] * 7,
}

# The fusion's five entry points share one parameter order; each leaves out the fields it does not have.  (field, ctype, the entry
# points that carry it, by the suffix of "pe_proben_fuse_batch"): SIGNATURES and fusion.fuse_batch's argument lists both come from here.
_EVERY = ("", "_logp", "_pooled", "_posterior", "_presence")
_LOGP, _WIDE = _EVERY[1:], _EVERY[2:]
FUSE_FIELDS = (
    [(f, c_void_p, _EVERY) for f in ("boxes", "scores", "probs", "vars", "classes")] + [("row_source", c_void_p, _WIDE)] +
    [(f, c_void_p, _EVERY) for f in ("offsets", "row_counts", "passthrough")] + [(f, c_int, _EVERY) for f in ("B", "K", "max_rows")] +
    [("score_mode", c_int, ("",)), ("box_mode", c_int, _EVERY)] + [(f, c_double, _EVERY) for f in ("thr", "fw", "fh")] +
    [("log_prior", c_void_p, _LOGP), ("pool_weights", c_void_p, _WIDE), ("presence", c_void_p, ("_presence",)), ("num_detectors", c_int, _WIDE)] +
    [(f, c_void_p, _EVERY) for f in ("out_boxes", "out_scores", "out_classes", "out_keep", "out_counts")] + [("out_cluster", c_void_p, _WIDE)] +
    [(f, c_void_p, _WIDE[1:]) for f in ("out_log_posterior", "out_vars", "out_members")] + [("out_pattern", c_void_p, ("_presence",)), ("stream", c_void_p, _EVERY)])
# entry point -> the fields it takes, in its parameter order; its argtypes are the same selection of the ctypes
FUSE_ORDER = {"pe_proben_fuse_batch" + e: [f for f, _, entries in FUSE_FIELDS if e in entries] for e in _EVERY}
SIGNATURES.update({"pe_proben_fuse_batch" + e: [t for _, t, entries in FUSE_FIELDS if e in entries] for e in _EVERY})
_RESTYPE = {"pe_last_error": ctypes.c_char_p, "pe_nms_scratch_bytes": ctypes.c_size_t, "pe_rpn_scratch_bytes": ctypes.c_size_t,
             "pe_bneck64_packed_bytes": ctypes.c_size_t, "pe_test_conv_variant": ctypes.c_char_p}


# exported for tests/ and scripts/ only (csrc/test_hooks.h) - not in include/proben_hip.h
TEST_HOOKS = {"pe_test_set_conv_policy": [c_int, c_int], "pe_test_get_conv_policy": [], "pe_test_conv_variant": [c_int] * 10 + [ctypes.c_int64], "pe_test_set_wd9_mode": [c_int], "pe_test_wd9_takes": [c_int] * 5, "pe_test_wd9_head_takes": [c_int] * 3, "pe_test_set_wd9_wgs": [c_int, c_int], "pe_test_set_ring_wgs": [c_int], "pe_test_set_roi_fast": [c_int], "pe_test_set_nms_presorted": [c_int],
              "pe_test_pdq_terms": [c_void_p] * 4 + [ctypes.c_int64] + [c_void_p] * 3}


class HipLibraryError(RuntimeError):
    pass


def lib():
    """The loaded library; raises HipLibraryError when it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  proben_amd has no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        L.pe_last_error.restype = ctypes.c_char_p
        L.pe_last_error.argtypes = []
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header/library mismatch
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, ctypes.c_int)
        _lib = L
    return _lib


LAB_HOOKS = {"pe_test_set_ring_ablation": [c_int]}     # exported by the LAB build only (`python -m proben_amd.build --lab`, -DPE_LAB)


def test_hooks():
    """The library with the measurement hooks of csrc/test_hooks.h typed (tests/ and scripts/ only)."""
    L = lib()
    for name, args in LAB_HOOKS.items():
        if hasattr(L, name):
            getattr(L, name).argtypes, getattr(L, name).restype = args, ctypes.c_int
    for name, args in TEST_HOOKS.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = args, _RESTYPE.get(name, ctypes.c_int)
    return L


def check(status, what):
    if status != 0:
        raise HipLibraryError(f"{what} failed ({status}): {lib().pe_last_error().decode()}")


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipLibraryError("proben_amd kernels need device tensors (MODEL.DEVICE=cuda); got a CPU tensor. "
                                  "There is no CPU fallback in the product path.")


def ptr(t):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous"
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
