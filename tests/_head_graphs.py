"""Small hand-written head graphs for byolo.train.HeadTrainer (csrc/train_heads.hip), for tests/test_train_heads_edges_gpu.py and
tests/test_train_heads_edges_cpu.py: a narrow backbone (tests/_layer_ref.py `stem`), byolo_mark_backbone_end, and a head whose channel
counts, grid and batch size land on the guards of the kernels that the real YOLOv3 heads reach at no image size -- each case's comment
names them.  The float64 reference of such a graph is tests/_heads_ref.py walking Graph.topology(); it costs milliseconds.

Vocabulary (csrc/train_heads.hip): M = B * h * w pixels (rows of forward / dgrad, the REDUCTION of wgrad); Kred = ks * ks * Cin the
reduction of forward (ks * ks * Cout that of dgrad), in steps of BK = 16; Kc = ks * ks * Cin the ROWS of wgrad, in tiles of 128 and
groups of 8; N = the columns, in tiles of 128 and groups of 8; a wgrad slice = the pixels one block of blockIdx.z reduces."""
import collections

import numpy as np

import _layer_ref as R

Prior = collections.namedtuple("Prior", "h w")
BM = BN_TILE = 128
BK = 16
RED_BLOCKS = 128
STEP_GOLD = 0x9E3779B97F4A7C15


class _Ref:
    def __init__(self, index):
        self.index = index


class DetLayer:
    def __init__(self, d, aleatoric_loss):
        self.h, self.w, self.priors, self.aleatoric_loss = d["H"], d["W"], [Prior(*p) for p in R.PRIORS], aleatoric_loss
        self._raw_ref = _Ref(d["idx"])


class Model:
    """what HeadTrainer asks of a lib_yolo model: .engine, .det_layers (h, w, priors, aleatoric_loss, _raw_ref.index), .finalize()"""

    def __init__(self, engine, g, aleatoric_loss):
        self.engine = engine
        self.det_layers = [DetLayer(d, aleatoric_loss) for d in g.L[g.first:] if d["op"] == "det"]

    def finalize(self):
        if not self.engine.finalized:
            self.engine.finalize()
        return self


Case = collections.namedtuple("Case", "H W B cls_cnt kind aleatoric_loss downs head expect")


# ---- the heads -------------------------------------------------------------------------------------------------------------------
def _ragged(g, kind):
    """3x3 64->40 +dropout, 1x1 40->24 +dropout, 3x3 24->20, detection.  Forward Kred 576 / 40 / 216 / 20 (40, 216 and 20 end inside
    a BK step); wgrad rows Kc 576 (4 row tiles + 64), 40, 216 (1 + 88) and 20 (no multiple of 8: rows 16 .. 19 through the scalar
    im2col8); dgrad (b, c, det; a's input is frozen) Kred 24 / 180 / 21 with "Cin" = 24 / 20 / 21 -- the 3x3 at 20 channels is the
    scalar im2col8 in a 3x3; N = 40, 24, 20 (scalar B tile: 20 & 7) and 21; dropout tensors of M * 40 and M * 24 elements"""
    g.conv("a", 40, 3, drop=True)
    g.conv("b", 24, 1, drop=True)
    g.conv("c", 20, 3)
    g.det("det", kind)


def _wide_n(g, kind):
    """1x1 64->136 = one column tile + 8, detection with N = 3 * (5 + cls_cnt): 255 = 128 + 127 at 80 classes -- whose dgrad has
    Cin = 255 (scalar im2col8) and Kred = 255"""
    g.conv("a", 136, 1)
    g.det("det", kind)


def _wide_c(g, kind):
    """264 channels: the `c += blockDim.x` loops of drop_stats_partial / bn_bwd_partial / colsum_partial and the second block of
    stats_final / bn_bwd_final; three column tiles (128 + 128 + 8)"""
    g.conv("a", 264, 1)
    g.det("det", kind)


def _views(g, kind):
    """low grid 5 x 7 (`w`, `lo`), high grid 10 x 14 (the frozen tap `s4`):
      a    a convolution fed by an upsample alone (gather n = 1, sh = 1; scatter of four children)
      b    concat [frozen tap, upsampled head tensor]: the trainable part at c_off = 32; `lo` is then read through TWO views, the
           second scatter into it runs with accumulate = 1
      c    concat of two head tensors, both trainable (scatter at c_off = 0 and c_off = 16); 3x3 with Cin = 28: the scalar
           im2col8 in a 3x3 forward and in wgrad's rows, Kred = Kc = 252 = 15 * 16 + 12
      c is read by det1 directly, by d directly (plain dgrad, accumulate = 1) and by e through a concat (scatter, the first writer)
      det3 reads the frozen tap directly: wgrad only, no dgrad"""
    g.conv("lo", 24, 1)
    g.up("up")
    g.conv("a", 16, 3)
    g.route("cat_b", ["s4", "up"])
    g.conv("b", 12, 1)
    g.route("cat_c", ["a", "b"])
    g.conv("c", 20, 3)
    g.det("det1", kind)
    g.route("c_again", ["c"])
    g.conv("d", 12, 1)
    g.route("cat_e", ["c", "d"])
    g.conv("e", 8, 1)
    g.det("det2", kind)
    g.route("tap", ["s4"])
    g.det("det3", kind)


def _thin(g, kind):
    """3x3 64->16, 1x1 16->8, detection: on a 1 x 3 grid the 3x3 taps have no row above or below; on the 1 x 1 grid with B = 1
    M = 1 -- batch variance 0, stats_final's Bessel guard, every gradient through a BN exactly zero apart from the L2 term"""
    g.conv("a", 16, 3)
    g.conv("b", 8, 1)
    g.det("det", kind)


# name -> Case.  Image sizes: grid << downs (stride 2 needs even grids: 160 x 224 reaches 5 x 7 as 10 x 14 -> 5 x 7, 96 x 160 reaches
# 3 x 5 as 6 x 10 -> 3 x 5).  expect: the raggedness the case is written for, asserted by test_train_heads_edges_cpu.py.
CASES = {
    "ragged M=35": Case(160, 224, 1, 2, 0, False, 5, _ragged, dict(
        M=35, slices={"a": 1, "b": 1, "c": 1, "det": 1}, Kc={"a": 576, "b": 40, "c": 216, "det": 20}, N={"a": 40, "b": 24, "c": 20, "det": 21},
        masks=[1400, 840])),
    # M = 385 = 3 * 128 + 1: a one-row tile behind three full ones; two wgrad slices of 208 + 177 pixels
    "ragged M=385": Case(160, 224, 11, 2, 0, False, 5, _ragged, dict(
        M=385, slices={"a": 2, "b": 2, "c": 2, "det": 2}, last_slice=177, masks=[15400, 9240])),
    # M = 525 = 4 * 128 + 13: three wgrad slices of 176 + 176 + 173 pixels
    "ragged M=525": Case(160, 224, 15, 2, 0, False, 5, _ragged, dict(
        M=525, slices={"a": 3, "b": 3, "c": 3, "det": 3}, last_slice=173, masks=[21000, 12600])),
    "N=255 cls=80": Case(96, 160, 3, 80, 0, False, 5, _wide_n, dict(M=45, N={"a": 136, "det": 255}, Kc={"a": 64, "det": 136})),
    "N=18 cls=1": Case(96, 160, 3, 1, 0, False, 5, _wide_n, dict(M=45, N={"a": 136, "det": 18})),
    "aleatoric N=36 cls=1": Case(96, 160, 3, 1, 1, True, 5, _wide_n, dict(M=45, N={"a": 136, "det": 36})),
    "264 channels": Case(96, 160, 3, 2, 0, False, 5, _wide_c, dict(M=45, N={"a": 264, "det": 21})),
    "views": Case(160, 224, 2, 2, 0, False, 5, _views, dict(M=280)),
    "grid 1x3": Case(32, 96, 3, 2, 0, False, 5, _thin, dict(M=9)),
    "grid 1x1 M=1": Case(32, 32, 1, 2, 0, False, 5, _thin, dict(M=1)),
}
DROPOUT_CASES = [n for n, c in CASES.items() if c.head is _ragged]


def build(name, eng=None):
    """the case's Graph (with `eng`: built into that handle as well)"""
    c = CASES[name]
    g = R.Graph(c.H, c.W, c.B, 1, eng=eng, cls_cnt=c.cls_cnt)
    R.stem(g, c.downs, 64)
    g.mark()
    c.head(g, c.kind)
    return g


def variant_of(c):
    return "yolov3" if c.kind == 0 else "yolov3_aleatoric"       # (tests/_heads_ref.py reads the loss's form off this name)


def head_names(g):
    """the trainable variables in creation order, and the moving statistics of the head"""
    names = list(g.shapes)[g.n_backbone_shapes:]
    return [n for n in names if "/moving_" not in n], [n for n in names if "/moving_" in n]


def head_convs(g):
    return [d for d in g.L[g.first:] if d["op"] in ("conv", "det")]


def boxes_for(name, n=4):
    c = CASES[name]
    rng = np.random.default_rng(R.case_seed(name) + 1)
    boxes = np.zeros((c.B, n, 4), np.float32)
    for b in range(c.B):
        for k in range(n):
            y0, x0 = rng.uniform(0.0, 0.6, 2)
            hh, ww = rng.uniform(0.1, 0.4), rng.uniform(0.08, 0.4)
            boxes[b, k] = [y0, x0, min(y0 + hh, 1.0), min(x0 + ww, 1.0)]
    return boxes, rng.integers(0, c.cls_cnt, (c.B, n)).astype(np.int32)


def masks_for(name, g):
    rng = np.random.default_rng(R.case_seed(name) + 2)
    return [rng.random(g.tensor_shape(d["idx"])) >= R.DROP_PROB for d in g.L[g.first:] if d.get("drop") is not None]


def stream_masks(g, seed, step):
    """the library's own dropout stream of a step: oracle.rng.keep_mask(seed + step * 0x9E3779B97F4A7C15 mod 2^64, ordinal, shape)"""
    from oracle import rng
    sk = (int(seed) + int(step) * STEP_GOLD) & (2 ** 64 - 1)
    return [rng.keep_mask(sk, d["drop"], g.tensor_shape(d["idx"]), R.DROP_PROB) for d in g.L[g.first:] if d.get("drop") is not None]


def cpu_gt(name, g):
    """ground truth of boxes_for(name) from the CPU restatement (oracle/train_ref.py encode_boxes), per detection layer"""
    from oracle import train_ref
    boxes, labels = boxes_for(name)
    layers = [(d["H"], d["W"], list(R.PRIORS)) for d in g.L[g.first:] if d["op"] == "det"]
    per_image = [train_ref.encode_boxes(boxes[b], labels[b], layers, 0.7) for b in range(boxes.shape[0])]
    return [{k: np.stack([img[l][k] for img in per_image]) for k in per_image[0][l]} for l in range(len(layers))]


def synthetic_taps(name, g):
    """float32 taps of the case's shapes for the CPU test: what a leaky-ReLU layer of the backbone hands over, of order one"""
    rng = np.random.default_rng(R.case_seed(name) + 3)
    taps = {}
    for d in head_convs(g):
        for i, _, _ in d["src"]:
            if i < g.first and i not in taps:
                v = rng.standard_normal(g.tensor_shape(i)).astype(np.float32)
                taps[i] = np.maximum(v, 0.1 * v)
    return taps


def reference(name, g, params, taps, gt, masks, dtype, defect=None):
    """tests/_heads_ref.py grads on this graph: (gradients, losses, raw outputs, batch statistics, {layer: head activation})"""
    import _heads_ref as hr
    c = CASES[name]
    acts = {}
    return hr.grads(params, taps, variant_of(c), gt, c.cls_cnt, masks, c.aleatoric_loss, dtype=dtype, all_params=params,
                    topo=g.topology(), first=g.first, names=head_names(g)[0], drop_prob=R.DROP_PROB, defect=defect, acts=acts) + (acts,)


# ---- the planner's wgrad slices (csrc/train_heads.hip trainer_plan) and the edges of a case -----------------------------------------
def plan_slices(M, Kc, Cout):
    """tiles = ceil(Kc / 128) * ceil(Cout / 128);  slices = max(1, min(ceil(1024 / tiles), ceil(M / 256))), fewer while the partial
    buffer slices * Kc * Cout * 4 exceeds 256 MB;  kslice = ceil(ceil(M / slices) / 16) * 16;  slices = ceil(M / kslice).
    Returns (slices, kslice, pixels of the last slice)."""
    tiles = -(-Kc // BM) * -(-Cout // BN_TILE)
    slices = max(1, min(-(-1024 // tiles), -(-M // 256)))
    while slices > 1 and slices * Kc * Cout * 4 > (256 << 20):
        slices -= 1
    ksl = -(-(-(-M // slices)) // BK) * BK
    slices = -(-M // ksl)
    return slices, ksl, M - (slices - 1) * ksl


def edges(g):
    """per head convolution: M, Kred of forward and dgrad, Kc, N, the planned slices -- what the guards of gemm_f32_kernel see"""
    out = {}
    for d in head_convs(g):
        M = g.B * d["H"] * d["W"]
        Kc = d["k"] * d["k"] * d["Cin"]
        s, ksl, last = plan_slices(M, Kc, d["C"])
        out[d["name"]] = dict(M=M, Kc=Kc, Kred=Kc, Kred_dgrad=d["k"] * d["k"] * d["C"], N=d["C"], Cin=d["Cin"], slices=s, kslice=ksl,
                              last_slice=last, parts=len(d["src"]), up=[u for _, u, _ in d["src"]],
                              frozen=[i < g.first for i, _, _ in d["src"]])
    return out


# ---- the bounds of tests/test_train_heads_gpu.py, in one place for the device test and the defect test ---------------------------------
def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def ratios(got, ref64, g32):
    """got: dict(raw=[...], losses={...}, grads={...}[, acts={layer: array}]) of a device run (or of a defective restatement);
    ref64 = reference(..., float64), g32 = the float32 reference's gradients.  {quantity: (error in units of its bound, max |err|,
    max |ref|)}: raw outputs and activations |err| <= 1e-4 * max(1, |ref|) per element, losses 1e-5 * |ref|, every gradient tensor
    max |err| <= max(1e-4 * max |ref|, 2 * d32).  A NaN / inf anywhere is an infinite error."""
    g64, l64, raw64 = ref64[:3]
    out = {}

    def elementwise(key, dev, ref):
        dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
        assert dev.shape == ref.shape, (key, dev.shape, ref.shape)
        err = np.abs(dev - ref)
        out[key] = (_ratio(err, 1e-4 * np.maximum(1.0, np.abs(ref))), float(np.nanmax(err)), float(np.abs(ref).max()))
    for k, (dev, ref) in enumerate(zip(got["raw"], raw64)):
        elementwise("raw %d" % k, dev, ref.numpy() if hasattr(ref, "numpy") else ref)
    for k, dev in got.get("acts", {}).items():
        elementwise("activation %d" % k, dev, ref64[4][k].numpy())
    for key, ref in l64.items():
        out[key] = (_ratio(abs(got["losses"][key] - ref), 1e-5 * abs(ref)), abs(got["losses"][key] - ref), abs(ref))
    assert list(got["grads"]) == list(g64), (list(got["grads"]), list(g64))
    for n, dev in got["grads"].items():
        ref = g64[n]
        d32 = np.abs(g32[n].astype(np.float64) - ref).max()
        err = np.abs(np.asarray(dev, np.float64) - ref)
        out["grad " + n] = (_ratio(err.max() if np.isfinite(err).all() else np.inf, max(1e-4 * np.abs(ref).max(), 2 * d32)),
                            float(np.nanmax(err)), float(np.abs(ref).max()))
    return out
