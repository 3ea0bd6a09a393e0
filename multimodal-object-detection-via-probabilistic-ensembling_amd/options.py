"""The fusion's options as one object: FusionOptions is built once - by an entry point from its keywords, by a caller who hands it on as
`options=`, or from the command line (from_args) - and is what fusion.py, late_fusion.py and pipeline.py read.  It applies the
combination rules (fusion._check_mode, the one statement of them), validates every value (calibration.check_*), supplies the
temperature default of "probEn-log", knows which derived facts follow (logp, needs_row_source, needs_cluster, the detector count) and
uploads what the kernels take from the device, once per device (on)."""
from collections import namedtuple

import numpy as np
import torch

from . import calibration

Uploaded = namedtuple("Uploaded", "log_prior pool_weights presence box_correlation")


def _uploaded(value):
    return isinstance(value, torch.Tensor) and value.is_cuda


def log_class_prior(class_prior, num_columns, device):
    """class_prior (K + 1 probabilities, background last; calibration.check_class_prior validates and normalises) -> the DEVICE
    f64 [K + 1] log-prior pe_proben_fuse_batch_logp takes.  None -> None (uniform).  A CUDA tensor is taken as the result of an
    earlier call."""
    if class_prior is None:
        return None
    if _uploaded(class_prior):
        if class_prior.dtype != torch.float64 or tuple(class_prior.shape) != (num_columns,):
            raise ValueError(f"log-prior tensor {tuple(class_prior.shape)} {class_prior.dtype} is not float64 [{num_columns}]")
        return class_prior.contiguous()
    return torch.from_numpy(np.log(calibration.check_class_prior(class_prior, num_columns))).to(device)


def pool_weight_tensor(pool_weights, num_detectors, device):
    """pool_weights (one exponent per detector; calibration.check_pool_weights validates: finite, >= 0, not all 0) -> the DEVICE f64
    [num_detectors] tensor pe_proben_fuse_batch_pooled takes.  None -> None.  A CUDA tensor is taken as the result of an earlier call."""
    if pool_weights is None:
        return None
    if _uploaded(pool_weights):
        if pool_weights.dtype != torch.float64 or tuple(pool_weights.shape) != (num_detectors,):
            raise ValueError(f"pool-weight tensor {tuple(pool_weights.shape)} {pool_weights.dtype} is not float64 [{num_detectors}]")
        return pool_weights.contiguous()
    return torch.tensor(calibration.check_pool_weights(pool_weights, num_detectors, "pool_weights"), dtype=torch.float64).to(device)


# fusion.py re-exports the two helpers above (their callers know them as fusion.log_class_prior / fusion.pool_weight_tensor) and this
# module reads fusion's mode tables and rules when an object is built: each imports the other, so this import comes after the helpers
from . import fusion as F  # noqa: E402


def checked(name, value, num_detectors, who):
    """One per-detector option's host value -> its validated form, with the messages the entry points have always given (`who` names
    the entry point).  None stays None; a CUDA tensor is taken as uploaded (on() checks its dtype and shape)."""
    D = num_detectors
    if value is None:
        return None
    if _uploaded(value):
        if name == "pool_weights" and D is not None and value.numel() != D:
            raise ValueError(f"{who}: {value.numel()} pool weights for {D} detectors")
        return value
    if name == "temperatures":
        value = [float(t) for t in value]
        if D is not None and len(value) != D:
            raise ValueError(f"{who}: {len(value)} temperatures for {D} detectors")
        return value
    if name == "variance_scales":
        return calibration.check_variance_scales(value, len(value) if D is None else D, who)
    if name == "pool_weights":
        return calibration.check_pool_weights(value, len(value) if D is None else D, who)
    if name == "presence":
        return calibration.check_presence(value, D, None, f"{who}: presence")
    if name == "wbf_weights":
        return calibration.check_wbf_weights(value, len(value) if D is None else D, who)
    assert name == "box_correlation", name
    return calibration.check_box_correlation(value, D, f"{who}: box_correlation")


class FusionOptions:
    """score_fusion / box_fusion and the calibration options of the fusion.  D = the number of detectors, K = the number of classes.

    temperatures     one T per detector: the rows' probabilities and scores are softmax(class_logits / T) in float64 instead of the
                     detectors' own float32 prob_score / scores.  "probEn-log" always fuses from logits: None = 1.0 per detector there.
    class_prior      ("probEn-log" only) K + 1 probabilities, background last, normalised here; None = uniform.  p(y)^(m-1) is divided
                     out of a cluster of m rows.  A CUDA tensor is taken as the uploaded LOG-prior (fusion.log_class_prior).
    variance_scales  one s per detector: the rows' variances are (double)var * s, one multiply.  They weight the member boxes of
                     box_fusion "v-avg" and "c-avg" and nothing else.
    pool_weights     ("probEn-log" only) one exponent w_d >= 0 per detector, not all 0: the logarithmic opinion pool
                     a_j = sum_t w_d(t) log p_t[j] - (W - 1) log prior_j; every weight 1 is "probEn-log" bit for bit.  A row's detector
                     comes from row_source.  The result then also holds "cluster" i32 [Ntot], the output row of the cluster each input
                     row ended in (-1: it left the pool without one; -2 where nothing was written: counts == -1, padding).
    with_posterior   ("probEn-log" only) the result also holds "log_posterior" f64 [Ntot, K+1] (the fused rows' normalised
                     log-posterior), "vars" f64 [Ntot] (the fused boxes' variance under the box rule) and "members" i32 [Ntot] (rows in
                     the cluster), indexed like "scores"; rows nothing was written to hold NaN / NaN / 0.
    presence         ("probEn-log" only) a table [2^D][K+1]: the fused columns gain presence[P][j], P the OR of (1 << source) over the
                     cluster's rows, last.  Clusters of one row and passthrough images are fused too (a silent detector is evidence as
                     well).  The result then also holds "pattern" i32 [Ntot] (the fused rows' P; -1 where nothing was written) and
                     "cluster".
    box_correlation  (box_fusion "c-avg", which is "probEn-log" only, and needs it) a matrix [D][D], one correlation of the normalised box
                     errors per detector pair: the fusion runs at "v-avg", then pe_box_gls_batch overwrites "boxes" - and "vars",
                     with_posterior - of the fused rows whose cluster has two or more rows with the generalised-least-squares mean and
                     the variance it really has.  A row whose source is outside [0, D) makes its cluster's box and variance NaN; a zero
                     matrix is "v-avg".  The result then also holds "cluster".
    wbf_weights      (score_fusion "wbf" with box_fusion "wbf": weighted boxes fusion, one method, so either half alone is refused) one
                     detector weight u_d >= 0, not all 0; None = 1.0 per detector.  A row counts with s = score * u_d(row), a row's
                     detector comes from row_source.  The method reads no variance, probability or logit: class_prior, pool_weights,
                     presence, with_posterior, box_correlation and variance_scales are refused beside it; temperatures stay legal (they
                     rebuild the score ahead of any fusion).  The result holds "cluster", "members" and "skipped" and no "keep".
    wbf_skip         ("wbf" only) the score floor: rows with s < wbf_skip are skipped (s == wbf_skip is kept); None = 0.

    pool_weights, presence and box_correlation are also taken as the CUDA tensors on() returns (fusion.pool_weight_tensor,
    calibration.presence_table, calibration.box_correlation_tensor).  num_detectors: D where the caller knows it (every per-detector
    value is then held to it); None takes it from the values, which must agree.  who: the entry point the messages name.
    What needs K + 1 (the prior's length, the table's width) is checked when on() is first given it."""

    def __init__(self, score_fusion="probEn", box_fusion="v-avg", temperatures=None, class_prior=None, variance_scales=None,
                 pool_weights=None, with_posterior=False, presence=None, box_correlation=None, num_detectors=None, who="FusionOptions",
                 wbf_weights=None, wbf_skip=None):
        F._check_mode(score_fusion, class_prior, who, pool_weights, with_posterior, presence, box_fusion, box_correlation,
                      variance_scales, wbf_weights, wbf_skip)
        self.score_fusion, self.box_fusion, self.with_posterior, self.who = score_fusion, box_fusion, bool(with_posterior), who
        self.logp, self.cavg, self.wbf = score_fusion == F.LOGP, box_fusion == F.CAVG, score_fusion == F.WBF
        D = num_detectors
        self.temperatures = checked("temperatures", temperatures, D, who)
        self.box_correlation = checked("box_correlation", box_correlation, D, who)
        self.presence = checked("presence", presence, D, who)
        self.pool_weights = checked("pool_weights", pool_weights, D, who)
        # the given prior is what on() uploads (normalised once, there); the normalised copy is for reading and for named()
        self._prior = class_prior
        self.class_prior = class_prior if class_prior is None or _uploaded(class_prior) else calibration.check_class_prior(class_prior)
        self.variance_scales = checked("variance_scales", variance_scales, D, who)
        self.wbf_weights = checked("wbf_weights", wbf_weights, D, who)
        self.wbf_skip = calibration.check_wbf_skip(0.0 if wbf_skip is None else wbf_skip, who) if self.wbf else None
        n_w = None if self.pool_weights is None else len(self.pool_weights)
        n_c = None if self.box_correlation is None else int(self.box_correlation.shape[0])
        n_p = None if self.presence is None else calibration.presence_detectors(self.presence)
        if None not in (n_w, n_c) and n_w != n_c:
            raise ValueError(f"{who}: {n_w} pool weights beside a box correlation over {n_c} detectors")
        if None not in (n_w, n_p) and n_w != n_p:
            raise ValueError(f"{who}: {n_w} pool weights beside a presence table over {n_p} detectors")
        if None not in (n_c, n_p) and n_c != n_p:
            raise ValueError(f"{who}: a box correlation over {n_c} detectors beside a presence table over {n_p}")
        n_u = None if self.wbf_weights is None else len(self.wbf_weights)
        self.num_detectors = next((n for n in (D, n_w, n_c, n_p, n_u) if n is not None), None)
        if self.wbf and self.wbf_weights is None and self.num_detectors is not None:
            self.wbf_weights = checked("wbf_weights", [1.0] * self.num_detectors, self.num_detectors, who)
        if self.logp and self.temperatures is None and self.num_detectors is not None:
            self.temperatures = [1.0] * self.num_detectors
        self.needs_row_source = self.pool_weights is not None or self.presence is not None or self.cavg or self.wbf
        self.needs_cluster = self.needs_row_source
        self.fitted = set()         # from_args: the image ids the calibration file's temperatures were fitted on
        self._on = {}

    @classmethod
    def of(cls, options, who, num_detectors, score_fusion="probEn", box_fusion="v-avg", **keywords):
        """What an entry point works with: `options` as given, else one built from the entry point's own keywords.  Both: TypeError."""
        if options is None:
            return cls(score_fusion, box_fusion, num_detectors=num_detectors, who=who, **keywords)
        given = [k for k, v in keywords.items() if v is not None and v is not False]
        if score_fusion not in ("probEn", options.score_fusion) or box_fusion not in ("v-avg", options.box_fusion):
            given.insert(0, f"another fusion ({score_fusion}, {box_fusion})")
        if given:
            raise TypeError(f"{who}: options= was given together with {', '.join(given)}: the object carries them")
        if num_detectors is not None and options.num_detectors not in (None, num_detectors):
            raise ValueError(f"{who}: options for {options.num_detectors} detectors, {num_detectors} given")
        return options

    def replace(self, **changes):
        """A new object with some of the constructor's arguments changed; everything is validated again."""
        now = dict(score_fusion=self.score_fusion, box_fusion=self.box_fusion, temperatures=self.temperatures, class_prior=self._prior,
                   variance_scales=self.variance_scales, pool_weights=self.pool_weights, with_posterior=self.with_posterior,
                   presence=self.presence, box_correlation=self.box_correlation, num_detectors=self.num_detectors, who=self.who,
                   wbf_weights=self.wbf_weights, wbf_skip=self.wbf_skip)
        now.update(changes)
        return FusionOptions(**now)

    def on(self, device, num_columns=None):
        """The device side: Uploaded(log_prior f64 [K+1], pool_weights f64 [D], presence f64 [2^D, K+1], box_correlation f64 [D, D]), None
        for what was not given.  Uploaded at the first call for a device (and K + 1 = num_columns, which the prior and the table are
        held to) and kept: later calls return the same tensors.  A value that already is a CUDA tensor is checked for dtype and shape."""
        key = (torch.device(device), num_columns)
        if key not in self._on:
            D = self.num_detectors
            self._on[key] = Uploaded(
                None if self._prior is None else log_class_prior(self._prior, num_columns or len(self._prior), device),
                pool_weight_tensor(self.pool_weights, D, device),
                None if self.presence is None else calibration.presence_table(self.presence, D, num_columns or self.presence.shape[1], device),
                calibration.box_correlation_tensor(self.box_correlation, D, device))
        return self._on[key]

    def wbf_on(self, device):
        """The detector weights of "wbf" on the device, f64 [D]; uploaded at the first call for a device and kept."""
        key = (torch.device(device), "wbf")
        if key not in self._on:
            self._on[key] = torch.tensor(self.wbf_weights, dtype=torch.float64).to(device)
        return self._on[key]

    def named(self, names):
        """The result keys that name the calibration a run was made with; a run without any carries none of them."""
        res = {}
        if self.temperatures is not None:
            res["temperatures"] = dict(zip(names, self.temperatures))
        if self._prior is not None:
            res["class_prior"] = self._prior
        if self.variance_scales is not None:
            res["variance_scales"] = dict(zip(names, self.variance_scales))
        if self.pool_weights is not None:
            res["pool_weights"] = dict(zip(names, self.pool_weights))
        if self.presence is not None:
            res["presence"] = {"detectors": list(names), "table": self.presence.tolist()}
        if self.box_correlation is not None:
            res["box_correlation"] = {"detectors": list(names), "matrix": self.box_correlation.tolist()}
        if self.wbf:
            res["wbf_weights"] = dict(zip(names, self.wbf_weights))
            res["wbf_skip"] = self.wbf_skip
        return res

    @classmethod
    def from_args(cls, args, names, who="demo_probEn", say=print):
        """The options of a command line (opt.config_parser) for the detectors `names`: each from its flag, else from the --calibration
        file's entry, else none.  The file is loaded once.  Options that do not belong to the chosen fusion (class prior, pool weights and
        presence without "probEn-log"; box correlation without "c-avg") are not read at all, so a file that carries them serves every
        fusion ("wbf" reads the file's temperatures and nothing else).  What the file supplies beyond temperatures and prior is said through `say` (None: silent)."""
        path = getattr(args, "calibration", None)
        rec = calibration.load(path) if path is not None else {}
        logp, cavg, wbf = args.score_fusion == F.LOGP, args.box_fusion == F.CAVG, F.WBF in (args.score_fusion, args.box_fusion)

        def pick(key, parse, table, resolve, show):
            text = getattr(args, key, None)
            if text is not None:
                return parse(text, names)
            if table is None:
                return None
            value = resolve(table, names, path)
            if say is not None and show is not None:
                say(show(value))
            return value

        pairs = [(a, b) for a in range(len(names)) for b in range(a, len(names))]
        pattern = lambda p: "+".join(n for d, n in enumerate(names) if p >> d & 1)  # noqa: E731
        per_name = lambda vals: ", ".join(f"{n}={v:.6g}" for n, v in zip(names, vals))  # noqa: E731
        temps = pick("temperatures", calibration.parse_temperatures, rec.get("detectors"), calibration.resolve, None)
        prior = None
        if logp:
            prior = calibration.parse_class_prior(args.class_prior).tolist() if getattr(args, "class_prior", None) is not None \
                else rec.get("class_prior")
        scales = pick("variance_scales", calibration.parse_variance_scales,
                      calibration.load_variance(path) if path is not None and not wbf else None,
                      calibration.resolve_variance_scales, lambda v: f"variance scales of {path}: {per_name(v)}")
        pool = pick("pool_weights", calibration.parse_pool_weights, rec.get("pool_weights"), calibration.resolve_pool_weights,
                    lambda v: f"pool weights of {path}: {per_name(v)}") if logp else None
        presence = pick("presence", calibration.parse_presence, rec.get("presence"), calibration.resolve_presence,
                        lambda t: f"presence table of {path}: " + ", ".join(pattern(p) + "=" + ":".join(f"{v:.6g}" for v in t[p])
                                                                            for p in range(1, len(t)))) if logp else None
        corr = None
        if cavg:
            corr = pick("box_correlation", calibration.parse_box_correlation, rec.get("box_correlation"), calibration.resolve_box_correlation,
                        lambda m: f"box correlation of {path}: " + ", ".join(f"{names[a]}:{names[b]}={m[a, b]:.6g}" for a, b in pairs))
            if corr is None:
                raise ValueError("--box_fusion c-avg needs --box_correlation or a --calibration file that carries \"box_correlation\" "
                                 "(fit_temperature --with-box-correlation)")
        weights = calibration.parse_wbf_weights(args.wbf_weights, names) if getattr(args, "wbf_weights", None) is not None else None
        opts = cls(args.score_fusion, args.box_fusion, temps, prior, scales, pool, bool(getattr(args, "write_fused", None)) and not wbf,
                   presence, corr, num_detectors=len(names), who=who, wbf_weights=weights,
                   wbf_skip=getattr(args, "wbf_skip", None) if wbf else None)
        opts.fitted = set(rec.get("fitted_image_ids", []))
        return opts
