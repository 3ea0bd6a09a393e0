"""GeneralizedRCNN inference on MI355X: the whole Faster R-CNN R50/R101-FPN forward as a stream of
HIP kernel launches over a batch (no host synchronisation until results are read).

Mirrors the call contract of the reference's meta-architecture
(detectron2/modeling/meta_arch/rcnn.py:146-302): `model(list[dict])` with "image" = CHW float tensor in
cfg.INPUT.FORMAT channel order (already resized), optional "height"/"width" = output resolution, returning
`list[{"instances": Instances}]` with pred_boxes / scores / pred_classes (+ class_logits, prob_score, vars).
Stage by stage it replaces: preprocess_image :269-286, ResNet/FPN (backbone/resnet.py, fpn.py),
StandardRPNHead + RPN.forward (proposal_generator/rpn.py:74-187), find_top_rpn_proposals
(rpn_outputs.py:52-161), ROIPooler (poolers.py:180-235), FastRCNNConvFCHead + FastRCNNOutputLayers
(roi_heads/box_head.py:73-81, fast_rcnn.py:531-545), FastRCNNOutputs.inference (fast_rcnn.py:417-452)
and detector_postprocess (postprocessing.py:8-38).
"""
import ctypes
import math
from dataclasses import dataclass

import torch

from . import _lib
from . import layers as L
from .data import PairFrames
from .structures import Boxes, Instances
from .weights import PackedDetector

SCALE_CLAMP = math.log(1000.0 / 16)


@dataclass
class DetectorConfig:
    """The handful of cfg keys the inference path reads."""
    num_classes: int = 3
    input_format: str = "BGR"          # BGR | RGB | BGRT | BGRTTT
    pixel_mean: tuple = (103.53, 116.28, 123.675)
    pixel_std: tuple = (1.0, 1.0, 1.0)
    anchor_sizes: tuple = (32, 64, 128, 256, 512)
    aspect_ratios: tuple = (0.5, 1.0, 2.0)
    pre_nms_topk: int = 1000
    post_nms_topk: int = 1000
    rpn_nms_thresh: float = 0.7
    score_thresh: float = 0.5
    nms_thresh: float = 0.5
    detections_per_image: int = 100
    min_size_test: int = 800
    max_size_test: int = 1333
    output_logits: bool = True
    enable_gaussian_nll: bool = True
    fix_vars: bool = False
    var_voting: bool = False            # variance voting after the box-head NMS; needs the variance head
    var_voting_sigma_t: float = 0.025   # a starting value in the range He et al. sweep - a setting, not a parity claim
    size_divisibility: int = 32

    @property
    def in_channels(self):
        return {"BGR": 3, "RGB": 3, "BGRT": 4, "BGRTTT": 6}[self.input_format]


def cell_anchor_table(sizes, ratios):
    """generate_cell_anchors (modeling/anchor_generator.py:148-180): float64 closed form, stored as float32."""
    out = []
    for s in sizes:
        area = float(s) ** 2.0
        for r in ratios:
            w = math.sqrt(area / r)
            h = r * w
            out += [-w / 2.0, -h / 2.0, w / 2.0, h / 2.0]
    return out


class GeneralizedRCNN:
    def __init__(self, cfg: DetectorConfig, state_dict, device="cuda"):
        if cfg.var_voting and not cfg.enable_gaussian_nll:
            raise ValueError("var_voting (PROBEN.VAR_VOTING) weights every candidate box by the variance its own proposal row predicts: "
                             "it needs the variance head (MODEL.ROI_HEADS.ENABLE_GAUSSIANNLLOSS)")
        if cfg.var_voting and not (math.isfinite(cfg.var_voting_sigma_t) and cfg.var_voting_sigma_t > 0):
            raise ValueError(f"var_voting_sigma_t (PROBEN.VAR_VOTING_SIGMA_T) must be finite and > 0, got {cfg.var_voting_sigma_t}")
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("GeneralizedRCNN (MODEL.DEVICE=cuda) needs an MI355X; there is no CPU fallback "
                                       "in proben_amd (the CPU restatement lives in oracle/ for testing only).")
        _lib.lib()
        self.cfg = cfg
        self.device = torch.device(device)
        self.w = PackedDetector(state_dict, device, cfg.num_classes)
        self.depth = self.w.depth
        assert len(cfg.aspect_ratios) == 3, "kernels assume 3 anchors per cell"
        self._cells = (ctypes.c_float * (len(cfg.anchor_sizes) * 12))(*cell_anchor_table(cfg.anchor_sizes, cfg.aspect_ratios))
        self._reg_w = (ctypes.c_float * 4)(10.0, 10.0, 5.0, 5.0)
        self.training = False
        self.use_wd = True   # weights-direct 3x3 kernel where the geometry allows (A/B switch)
        self.fuse_tails = True   # conv2 + conv3 of a bottleneck in one launch where conv2 is 256 wide (A/B switch)
        self.fuse_pairs = True   # conv3 + shortcut of a 128 -> 512 block with the next block's conv1 in one launch: res3 (A/B switch)
        self.fuse_res2 = True    # res2 as the fused 64-wide bottleneck chain of csrc/bneck64.hip (A/B switch)

    def eval(self):
        return self

    def load_state_dict(self, state_dict, strict=True):
        """Re-pack a reference-format state dict into the device tensors the kernels read (what
        DetectionCheckpointer(model).load(path) ends in)."""
        w = PackedDetector(state_dict, self.device, self.cfg.num_classes)
        assert w.depth == self.depth or not strict, f"state dict is ResNet-{w.depth}, model was built as ResNet-{self.depth}"
        self.w, self.depth = w, w.depth
        return self

    def to(self, device):
        assert torch.device(device).type == "cuda", "proben_amd.GeneralizedRCNN lives on the GPU (no CPU fallback)"
        return self

    # ------------------------------------------------------------------ stages
    def _conv(self, x, conv, wd=None, **kw):
        """conv2d_nhwc of a (weight, bias) entry; a 3x3 with a fragment-ordered copy `wd` runs on the weights-direct kernel where that takes x."""
        w, b = conv
        if wd is not None and self.use_wd and kw.get("residual") is None and L.conv_wd_takes(x, w.shape[0]):
            return L.conv3x3_wd(x, wd, b, w.shape[0], relu=kw.get("relu", False), out=kw.get("out"), out_stride=kw.get("out_stride", 0))
        return L.conv2d_nhwc(x, w, b, **kw)

    def _named(self, x, name, **kw):
        return self._conv(x, self.w.convs[name], self.w.wd.get(name), **kw)

    def _bottom_up(self, x, prefix):
        """Stem, then every stage (weights.Stage) as its 64-wide chain or block by block.  Which routes a block CAN take was settled when
        the weights were packed; the A/B switches and the launch's size decide here."""
        fused = self.w.convs.get(prefix + ".bottom_up.stem.fused")
        if fused is not None and x.shape[1] % 4 == 0 and x.shape[2] % 4 == 0:
            x = L.stem_conv_pool(x, *fused)  # conv + ReLU + pool in one pass over HBM
        else:
            x = self._named(x, prefix + ".bottom_up.stem.conv1", kernel=7, stride=2, relu=True)
            x = L.maxpool3x3s2_nhwc(x)
        outs = []
        for si, stage in enumerate(self.w.stages[prefix]):
            if self.fuse_res2 and stage.chain64 is not None and L.bneck64_supported(*x.shape[:3]):
                x = self._chain64(x, stage)
            else:
                t1 = None   # a block's conv1 output where the previous block's pair launch has already produced it
                for blk in stage.blocks:
                    x, t1 = self._block(x, blk, t1)
            outs.append(x)
            hook = getattr(self, "stage_hook", None)
            if hook is not None:
                hook(si + 2)  # pipeline.py staggers the second detector's stream behind this point
        return outs  # res2..res5

    def _chain64(self, x, stage):
        """res2 in 1 + nb launches: conv1 of the first block, then per block 3x3 -> conv3 (+ shortcut) -> the next block's conv1; neither the
        64-channel intermediates, nor the shortcut convolution's output, nor a re-read of a block output by the next conv1 go through HBM."""
        t1 = self._conv(x, stage.blocks[0].conv1, kernel=1, relu=True)
        for c in stage.chain64:
            x, t1 = L.bneck64(t1, x, c["packed"], c["b2"], c["b3"], c["bsc"], c["b1n"])
        return x

    def _block(self, x, blk, t1):
        """The first route of pair > tail > plain that takes the block -> (its output, the NEXT block's conv1 output | None)."""
        sc = self._conv(x, blk.shortcut, kernel=1, stride=blk.stride) if blk.shortcut is not None else x
        o = t1 if t1 is not None else self._conv(x, blk.conv1, kernel=1, stride=blk.stride, relu=True)
        w3 = blk.conv3[0]
        if self.fuse_pairs and blk.pair is not None \
                and L.conv1x1_pair_supported(w3.shape[-1], w3.shape[0], blk.pair[0].shape[0], o.shape[0] * o.shape[1] * o.shape[2]):
            return self._pair(o, sc, blk)
        if self.use_wd and self.fuse_tails and blk.tail is not None and L.conv_wd_takes(o, 256, blk.tail[2]):
            return self._tail(o, sc, blk), None
        return self._plain(o, sc, blk), None

    def _pair(self, o, sc, blk):
        """conv2, then conv3 + shortcut + ReLU and the next block's conv1 + ReLU in one launch (res3): the output is not read back from HBM."""
        o = self._conv(o, blk.conv2, blk.wd, kernel=3, relu=True)
        return L.conv1x1_pair(o, *blk.conv3, sc, *blk.pair)

    def _tail(self, o, sc, blk):
        """conv2 + ReLU + conv3 + shortcut + ReLU in one launch (res4): the 256-channel intermediate stays on the chip."""
        return L.bottleneck_tail_wd(o, blk.wd, blk.conv2[1], blk.tail[0], blk.tail[1], sc, blk.tail[2])

    def _plain(self, o, sc, blk):
        o = self._conv(o, blk.conv2, blk.wd, kernel=3, relu=True)
        return self._conv(o, blk.conv3, kernel=1, relu=True, residual=sc, residual_mode=1)

    def _fpn(self, x, prefix="backbone", outs=None, ch_off=0, ch_total=256):
        """Returns [p2,p3,p4,p5,p6].  With `outs` given (middle fusion) the 3x3 output convs write their
        256 channels at channel offset ch_off of the preallocated [N,H,W,ch_total] tensors."""
        res = self._bottom_up(x, prefix)
        feats = [None] * 5
        prev = None
        for i in (5, 4, 3, 2):
            c = res[i - 2]
            if prev is None:
                prev = self._named(c, f"{prefix}.fpn_lateral{i}", kernel=1)
            else:
                prev = self._named(c, f"{prefix}.fpn_lateral{i}", kernel=1, residual=prev, residual_mode=2)
            if outs is None:
                feats[i - 2] = self._named(prev, f"{prefix}.fpn_output{i}", kernel=3)
            else:
                view = outs[i - 2].view(-1)[ch_off:]
                self._named(prev, f"{prefix}.fpn_output{i}", kernel=3, out=view, out_stride=ch_total)
                feats[i - 2] = outs[i - 2]
        if outs is None:
            feats[4] = L.subsample2_nhwc(feats[3])
        return feats

    def _input_plan(self, sizes):
        """For resized images of `sizes`: per NHWC4 batch to fill, the keywords ch0 / nch / mean / std of its pack launch; the padded (H, W)."""
        cfg = self.cfg
        C, d = cfg.in_channels, cfg.size_divisibility
        mean = list(cfg.pixel_mean)
        std = list(cfg.pixel_std) + [cfg.pixel_std[-1]] * (C - len(cfg.pixel_std))
        assert len(mean) == C, f"PIXEL_MEAN needs {C} entries for INPUT.FORMAT {cfg.input_format}"
        # BGRTTT: the thermal half divides by PIXEL_STD[:3] (meta_arch/rcnn.py:63-66)
        groups = [dict(ch0=c0, nch=n, mean=mean[c0:c0 + n], std=std[:n]) for c0, n in ([(0, min(C, 4))] if C <= 4 else [(0, 3), (3, 3)])]
        return groups, tuple((max(s[i] for s in sizes) + d - 1) // d * d for i in (0, 1))

    def _preprocess(self, images, resize_to=None):
        """images: list of device tensors.  CHW float32 (reference contract, already resized) or HWC uint8 /
        float32 raw frames (then `resize_to` = (h, w) applies ResizeShortestEdge's target on the GPU).
        Returns NHWC4 fp16 batch(es) and [(h, w)] of the resized, unpadded images."""
        C = self.cfg.in_channels
        if isinstance(images, PairFrames):
            return self._preprocess_pair(images, resize_to)
        if isinstance(images, torch.Tensor):  # one [N,H,W,C] (or [N,C,H,W] f32) batch of equally sized frames
            return self._preprocess_batch(images, resize_to)
        sizes, kinds = [], []
        for im in images:
            chw = im.dim() == 3 and im.shape[0] == C and im.dtype == torch.float32 and im.shape[2] != C
            kinds.append(2 if chw else (0 if im.dtype == torch.uint8 else 1))
            h, w = (im.shape[1], im.shape[2]) if chw else (im.shape[0], im.shape[1])
            sizes.append(tuple(resize_to) if (resize_to is not None and not chw) else (h, w))
        groups, (Hp, Wp) = self._input_plan(sizes)
        batches = [torch.empty((len(images), Hp, Wp, 4), dtype=torch.float16, device=self.device) for _ in groups]
        for g, x in zip(groups, batches):
            for i, im in enumerate(images):
                if kinds[i] == 0 and C == 3 and tuple(sizes[i]) != tuple(im.shape[:2]):
                    # 3-channel uint8 + resize: the reference goes through Pillow (transform.py:92-97) - exact restatement
                    L.preprocess_pack_pil_u8(im.contiguous(), x[i], flip_rgb=False, dst_hw=sizes[i], **g)
                else:
                    L.preprocess_pack(im.contiguous(), x[i], src_kind=kinds[i], flip_rgb=False, dst_hw=sizes[i], **g)
        return batches, sizes

    def _preprocess_batch(self, images, resize_to):
        C = self.cfg.in_channels
        N = images.shape[0]
        chw = images.dtype == torch.float32 and images.shape[1] == C and images.shape[3] != C
        kind = 2 if chw else (0 if images.dtype == torch.uint8 else 1)
        h, w = (images.shape[2], images.shape[3]) if chw else (images.shape[1], images.shape[2])
        size = tuple(resize_to) if (resize_to is not None and not chw) else (h, w)
        groups, (Hp, Wp) = self._input_plan([size])
        batches = [torch.empty((N, Hp, Wp, 4), dtype=torch.float16, device=self.device) for _ in groups]
        for g, x in zip(groups, batches):
            if kind == 0 and C == 3 and tuple(size) != (h, w):   # Pillow-exact resize (see _preprocess)
                L.preprocess_pack_pil_u8(images.contiguous(), x, flip_rgb=False, dst_hw=size, **g)
            else:
                L.preprocess_pack_batch(images.contiguous(), x, src_kind=kind, flip_rgb=False, dst_hw=size, **g)
        return batches, [size] * N

    def _preprocess_pair(self, pair, resize_to):
        """data.PairFrames: thermal_only (BGR) takes the thermal batch on the Pillow-exact route; early / middle fusion
        (BGRT / BGRTTT) build their stacked input from the two uint8 batches in one launch per output group."""
        cfg = self.cfg
        if cfg.input_format == "BGR":
            return self._preprocess_batch(pair.thermal, resize_to)
        if cfg.input_format not in ("BGRT", "BGRTTT"):
            raise ValueError(f"PairFrames feeds the thermal_only / early_fusion / middle_fusion detectors; INPUT.FORMAT "
                             f"{cfg.input_format} sees the RGB frame at its own size - give it the RGB batch itself")
        if pair.rgb is None:
            raise ValueError(f"INPUT.FORMAT {cfg.input_format} needs the RGB batch of the frame pairs")
        N, h, w = pair.thermal.shape[:3]
        size = tuple(resize_to) if resize_to is not None else (h, w)
        groups, (Hp, Wp) = self._input_plan([size])
        batches = [torch.empty((N, Hp, Wp, 4), dtype=torch.float16, device=self.device) for _ in groups]
        for g, x in zip(groups, batches):
            L.fusion_input_pack(pair.thermal.contiguous(), pair.rgb.contiguous() if g["ch0"] < 3 else None, x, dst_hw=size,
                                pad_multiple=cfg.size_divisibility, **g)
        return batches, [size] * N

    def _rpn(self, feats, sizes_dev, N, heads=None):
        """heads (tests): precomputed fp32 RPN head outputs [N,H,W,16] per level (3 objectness + 12 deltas) instead of
        running the head convolutions - lets the discrete chain be checked on the oracle's own fp32 numbers."""
        cfg = self.cfg
        hw, strides = [], [4, 8, 16, 32, 64]
        if heads is None:
            heads = []
            fused = self.w.rpn_head_fused if self.use_wd else None
            for f in feats:
                if fused is not None and L.conv_wd_takes(f, 256):
                    # StandardRPNHead in one launch: the 256-channel ReLU'd map never goes to HBM
                    heads.append(L.conv3x3_wd_rpn_head(f, self.w.wd["rpn.conv"], self.w.convs["rpn.conv"][1], fused[0], fused[1]))
                    continue
                t = self._named(f, "rpn.conv", kernel=3, relu=True)
                heads.append(L.conv2d_nhwc(t, *self.w.convs["rpn.head"], kernel=1, out_f32=True, cout=15, cout_store=15, out_stride=16))
        feats = heads
        for f in feats:
            hw += [f.shape[1], f.shape[2]]
        nl = len(feats)
        topk = [min(cfg.pre_nms_topk, f.shape[1] * f.shape[2] * 3) for f in feats]
        ncand = sum(topk)
        dev = self.device
        cb = torch.empty((N, ncand, 4), dtype=torch.float32, device=dev)
        cs = torch.empty((N, ncand), dtype=torch.float32, device=dev)
        cl = torch.empty((N, ncand), dtype=torch.int32, device=dev)
        cv = torch.empty((N, ncand), dtype=torch.uint8, device=dev)
        ptrs = (ctypes.c_void_p * nl)(*[h.data_ptr() for h in heads])
        hw_c = (ctypes.c_int32 * (2 * nl))(*hw)
        sbytes = _lib.lib().pe_rpn_scratch_bytes(hw_c, nl, N)
        scratch = torch.empty((max(sbytes, 8),), dtype=torch.uint8, device=dev)
        st = _lib.lib().pe_rpn_select_topk(ptrs, hw_c, (ctypes.c_int32 * nl)(*strides[:nl]),
                                          self._cells, nl, N, 16, cfg.pre_nms_topk, _lib.ptr(sizes_dev), SCALE_CLAMP,
                                          _lib.ptr(cb), _lib.ptr(cs), _lib.ptr(cl), _lib.ptr(cv), ncand,
                                          _lib.ptr(scratch), sbytes, _lib.stream())
        _lib.check(st, "pe_rpn_select_topk")
        mode = 1 if ncand * 4 > 20000 else 0  # torchvision.batched_nms dispatch (GPU threshold)
        keep, kcnt = L.nms_batched_raw(cb, cs, cl, None, cv, cfg.rpn_nms_thresh, mode, cfg.post_nms_topk)
        props = torch.empty((N, cfg.post_nms_topk, 4), dtype=torch.float32, device=dev)
        plog = torch.empty((N, cfg.post_nms_topk), dtype=torch.float32, device=dev)
        st = _lib.lib().pe_gather_boxes(_lib.ptr(cb), _lib.ptr(cs), _lib.ptr(keep), _lib.ptr(kcnt), N, ncand,
                                       cfg.post_nms_topk, _lib.ptr(props), _lib.ptr(plog), _lib.stream())
        _lib.check(st, "pe_gather_boxes")
        return props, plog, kcnt, heads

    def _roi_heads(self, feats, props, pcnt, sizes_dev, out_dev, N, head=None):
        """head (tests): precomputed fp32 predictor outputs [N*P, head_stride] (K+1 logits, 4K deltas, log-variance)
        instead of ROIAlign + the FC layers."""
        cfg, w = self.cfg, self.w
        P = cfg.post_nms_topk
        K = cfg.num_classes
        dev = self.device
        pooled = None
        if head is None:
            C = feats[0].shape[3]
            pooled = L.roi_align_nhwc(feats[:4], props, scales=[1 / 4, 1 / 8, 1 / 16, 1 / 32], pooled=(7, 7),
                                      sampling_ratio=0, aligned=True, counts=pcnt, per_image=P, num_rois=N * P)
            x = L.linear_f16(pooled.view(N * P, 49 * C), w.fc1[0], w.fc1[1], relu=True)
            x = L.linear_f16(x, w.fc2[0], w.fc2[1], relu=True)
            head = L.linear_f16(x, w.predictor[0], w.predictor[1], out_f32=True, cout_store=w.head_cols, out_stride=w.head_stride)
        # a proposal can pass the threshold in at most ceil(1/thr) - 1 classes (softmax sums to 1): never size beyond that
        per_prop = min(K, max(1, int(math.ceil(1.0 / max(cfg.score_thresh, 1e-6))) - 1))
        cmax = min(P * per_prop, 16384)   # 16384 = pe_nms_batched's row limit; overflow is REPORTED (cand_total), not silent
        cb = torch.empty((N, cmax, 4), dtype=torch.float32, device=dev)
        cs = torch.empty((N, cmax), dtype=torch.float32, device=dev)
        cc = torch.empty((N, cmax), dtype=torch.int32, device=dev)
        cr = torch.empty((N, cmax, 2), dtype=torch.int32, device=dev)
        ccnt = torch.empty((N,), dtype=torch.int32, device=dev)
        ctot = torch.empty((N,), dtype=torch.int32, device=dev)
        probs = torch.empty((N, P, K + 1), dtype=torch.float32, device=dev)
        lib = _lib.lib()
        st = lib.pe_boxhead_candidates(_lib.ptr(head), w.head_stride, N, P, K, _lib.ptr(pcnt), _lib.ptr(props),
                                       _lib.ptr(sizes_dev), self._reg_w, SCALE_CLAMP, cfg.score_thresh, cmax,
                                       _lib.ptr(cb), _lib.ptr(cs), _lib.ptr(cc), _lib.ptr(cr), _lib.ptr(ccnt), _lib.ptr(ctot),
                                       _lib.ptr(probs), _lib.stream())
        _lib.check(st, "pe_boxhead_candidates")
        D = cfg.detections_per_image
        mode = 1 if cmax * 4 > 20000 else 0
        keep, kcnt = L.nms_batched_raw(cb, cs, cc, ccnt, None, cfg.nms_thresh, mode, D)
        fb = cb                      # the boxes finalize gathers: the candidates', or their variance-voted copy
        if cfg.var_voting:
            fb = torch.empty_like(cb)
            st = lib.pe_boxhead_var_vote(_lib.ptr(head), w.head_stride, N, P, K, cmax, D, _lib.ptr(cb), _lib.ptr(cc), _lib.ptr(cr),
                                         _lib.ptr(ccnt), _lib.ptr(keep), _lib.ptr(kcnt), cfg.var_voting_sigma_t, _lib.ptr(fb),
                                         _lib.stream())
            _lib.check(st, "pe_boxhead_var_vote")
        det = {
            "boxes": torch.empty((N, D, 4), dtype=torch.float32, device=dev),
            "scores": torch.empty((N, D), dtype=torch.float32, device=dev),
            "classes": torch.empty((N, D), dtype=torch.int32, device=dev),
            "class_logits": torch.empty((N, D, K + 1), dtype=torch.float32, device=dev),
            "prob_score": torch.empty((N, D, K), dtype=torch.float32, device=dev),
            "vars": torch.empty((N, D), dtype=torch.float32, device=dev),
            "rows": torch.empty((N, D), dtype=torch.int32, device=dev),
            "counts": torch.empty((N,), dtype=torch.int32, device=dev),
        }
        st = lib.pe_boxhead_finalize(_lib.ptr(head), w.head_stride, N, P, K, cmax, D, int(cfg.fix_vars), _lib.ptr(probs),
                                     _lib.ptr(fb), _lib.ptr(cs), _lib.ptr(cc), _lib.ptr(cr), _lib.ptr(keep), _lib.ptr(kcnt),
                                     _lib.ptr(sizes_dev), _lib.ptr(out_dev), _lib.ptr(det["boxes"]), _lib.ptr(det["scores"]),
                                     _lib.ptr(det["classes"]), _lib.ptr(det["class_logits"]), _lib.ptr(det["prob_score"]),
                                     _lib.ptr(det["vars"]), _lib.ptr(det["rows"]), _lib.ptr(det["counts"]), _lib.stream())
        _lib.check(st, "pe_boxhead_finalize")
        det["_head"] = head
        det["_pooled"] = pooled
        det["cand_total"], det["cand_max"] = ctot, cmax
        return det

    # ------------------------------------------------------------------ public API
    @torch.no_grad()
    def forward_batch(self, images, out_sizes=None, resize_to=None, keep_intermediates=False):
        """Batched device-resident forward.  images: list of device tensors (see _preprocess).
        out_sizes: list of (height, width) per image for the final rescale (default: resized size).
        Returns a dict of padded device tensors: boxes [N,D,4], scores, classes, class_logits,
        prob_score, vars, counts [N]."""
        N = images.shape[0] if isinstance(images, torch.Tensor) else len(images)   # list of frames or data.PairFrames
        batches, sizes = self._preprocess(images, resize_to)
        dev = self.device
        out_sizes = out_sizes if out_sizes is not None else sizes
        # [N,2] size tables live on the device and are cached by content: a pageable H2D copy per forward would make the
        # host wait for the stream (measured r02: 13 ms of host blocking per forward at batch 32)
        sizes_dev = self._size_table(sizes)
        out_dev = self._size_table(out_sizes)
        if self.w.middle_fusion:
            Hp, Wp = batches[0].shape[1], batches[0].shape[2]
            shapes = [(Hp // s, Wp // s) for s in (4, 8, 16, 32)]
            outs = [torch.empty((N, h, w, 512), dtype=torch.float16, device=dev) for h, w in shapes]
            # Q1: the reference's INFERENCE runs both halves through `backbone` (meta_arch/rcnn.py:243-244)
            self._fpn(batches[0], "backbone", outs, 0, 512)
            self._fpn(batches[1], "backbone", outs, 256, 512)
            feats = outs + [L.subsample2_nhwc(outs[3])]
        else:
            feats = self._fpn(batches[0], "backbone")
        props, plog, pcnt, heads = self._rpn(feats, sizes_dev, N)
        det = self._roi_heads(feats, props, pcnt, sizes_dev, out_dev, N)
        det["proposals"], det["proposal_logits"], det["proposal_counts"] = props, plog, pcnt
        det["image_sizes"], det["out_sizes"] = sizes, [tuple(s) for s in out_sizes]
        if keep_intermediates:
            det["_feats"], det["_rpn_heads"], det["_input"] = feats, heads, batches
        else:
            det.pop("_head", None)
            det.pop("_pooled", None)
        return det

    def _size_table(self, sizes):
        key = tuple((int(h), int(w)) for h, w in sizes)
        cache = self.__dict__.setdefault("_size_tables", {})
        t = cache.get(key)
        if t is None:
            if len(cache) > 64:
                cache.clear()
            t = torch.tensor(key, dtype=torch.int32).reshape(-1, 2).to(self.device)
            torch.cuda.current_stream(self.device).synchronize()   # shared by every stream from now on
            cache[key] = t
        return t

    def to_instances(self, det):
        """Device result dict -> list[{"instances": Instances}] (one host sync)."""
        counts = det["counts"].cpu().tolist()
        if "cand_total" in det and int(det["cand_total"].max()) > det["cand_max"]:
            raise RuntimeError(f"box head: {int(det['cand_total'].max())} (proposal, class) candidates pass SCORE_THRESH_TEST="
                               f"{self.cfg.score_thresh} on one image but the NMS stage holds {det['cand_max']}: detections would be "
                               "dropped in proposal order (the reference keeps all).  Raise the threshold or lower POST_NMS_TOPK_TEST.")
        cfg = self.cfg
        out = []
        for n, c in enumerate(counts):
            inst = Instances(tuple(det["out_sizes"][n]))
            inst.pred_boxes = Boxes(det["boxes"][n, :c])
            inst.scores = det["scores"][n, :c]
            inst.pred_classes = det["classes"][n, :c].to(torch.int64)
            if cfg.output_logits:
                inst.class_logits = det["class_logits"][n, :c]
                inst.prob_score = det["prob_score"][n, :c]
            if cfg.enable_gaussian_nll:
                inst.vars = det["vars"][n, :c].unsqueeze(1)
            out.append({"instances": inst})
        return out

    def inference(self, batched_inputs, do_postprocess=True):
        assert not self.training
        images = [x["image"].to(self.device) for x in batched_inputs]
        out_sizes = [(x.get("height", x["image"].shape[-2]), x.get("width", x["image"].shape[-1])) for x in batched_inputs]
        if not do_postprocess:
            out_sizes = None
        return self.to_instances(self.forward_batch(images, out_sizes))

    def __call__(self, batched_inputs):
        return self.inference(batched_inputs)
