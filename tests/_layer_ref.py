"""ONE layer of the convolution stack evaluated in isolation on the CPU, three ways, for tests/test_gpu_layer_f64.py and
tests/test_layer_ref_cpu.py:

    layer_eval(..., dtype=float64)   the exact value y64 of the layer function of lib_yolo/layers.py:533-613 on the given input, and the
                                     per-element magnitude  m = (|x| (*) |w|) * |dropout gain| * |bn scale| + |shift| + |residual|
    layer_eval(..., dtype=float32)   F: the same function in plain float32 (NCHW F.conv2d, as tests/test_gpu_layers.py::_ref_conv)
    layer_split(...)                 S: the arithmetic of the default precision (csrc/mfma_pipe.h) emulated: hi/lo fp16 pairs, the three
                                     products hi_x hi_w + hi_x lo_w + lo_x hi_w in fp32 -- directly or as Winograd F(2x2,3x3)
                                     (csrc/wino_split.hip) --, the epilogue in fp32, the output rounded to hi + lo

The input is the device's OWN input of that layer (Engine.layer_output: hi + lo is exact in fp32), so nothing accumulates from layer to
layer: the distance  E = max |y - y64| / m  is that of this layer's kernel and of nothing else.  The criterion of the device test is
E_device <= 4 * max(E_S, E_F): the device may differ from the emulation in the order of its sums (16-product MFMA blocks, K slices, the
Winograd fold) and in the two or three fp32 roundings of its epilogue, not by a lost correction term -- `mutant` builds six such one-line
defects into S, and test_layer_ref_cpu.py shows each of them at >= 4 x that bound on every shape the device test uses.

The fp32 mode (tests/test_gpu_layer_f64_fp32.py, tests/test_layer_ref_f32_cpu.py; CASES_F32 below) has F as its unit, and on a Winograd
layer max(W, F):

    layer_f32(..., wino=...)         W: the fp32 Winograd path of csrc/winograd.hip / wino_fused.hip restated -- V = B^T d B in fp32 adds,
                                     U = G g G^T in double rounded once, 16 products accumulated in fp32 over the input channels,
                                     Y = A^T M A in fp32 adds in the kernels' order, the fp32 epilogue
    MUTANTS_F32                      six one-line defects of F or W; the direct small-Cin kernels (both precisions) have as S an fp32
                                     convolution whose output is rounded to hi + lo

A layer's sources are a list of (NHWC tensor, upsampled): the two-source concat loader with its x2 nearest upsample (layers.py:578-592)
is part of the layer.  A stacked input is the caller's repeat_interleave(T, dim=0) (sample s = image * T + t, layers.py:595-597)."""
import torch
import torch.nn.functional as F

from oracle import rng

ACT_SCALE = 4.0          # activations: hi = RNE_f16(4 x), lo = RNE_f16(4 x - hi)
BN_EPS = 1e-5
CHUNK = 32               # input channels of one K-tile
MUTANT_CHUNK = 1         # the mutants touch input channels 32 .. 63
MUTANTS = {1: "lo_w zeroed for one 32-channel chunk at one tap",
           2: "lo_x zeroed for one chunk in the last image column",
           3: "left neighbour of column 0 wraps to the pixel before it in memory, for one tap",
           4: "residual added from its hi half only",
           5: "Winograd: V's lo plane zeroed at one of the 16 points for one chunk",
           6: "Winograd: the pad row / column of an odd grid takes the neighbouring pixels in memory"}


def _split(a, scale):
    a = a * scale
    hi = a.half().float()
    lo = (a - hi).half().float()
    return hi / scale, lo / scale


def weight_scale(w, dims=(0, 1, 2)):
    """one power of two per output channel (byolo_finalize): the channel's largest |w| in [2^13, 2^14)"""
    return torch.exp2(13 - torch.floor(torch.log2(w.abs().amax(dim=dims).clamp(min=1e-30))))


def conv_nhwc(x, w, stride):
    """NHWC x HWIO cross-correlation: SAME on stride 1; on stride 2 Darknet's pad of one row / column on top / left, then VALID
    (layers.py:616-635 on the even grids the builder accepts)."""
    k = w.shape[0]
    xn, wn = x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1)
    if stride == 2:
        y = F.conv2d(F.pad(xn, (1, 0, 1, 0)), wn, stride=2)
    else:
        y = F.conv2d(xn, wn, padding=(k - 1) // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def _split_conv(x, w, stride, conv=conv_nhwc, mutant=None):
    """The three-product convolution of the direct kernels (csrc/conv_igemm.hip)."""
    xh, xl = _split(x, ACT_SCALE)
    wh, wl = _split(w, weight_scale(w))
    c0 = min(MUTANT_CHUNK, x.shape[3] // CHUNK - 1) * CHUNK
    if mutant == 1:
        wl = wl.clone()
        wl[w.shape[0] // 2, w.shape[1] // 2, c0:c0 + CHUNK] = 0
    if mutant == 2:
        xl = xl.clone()
        xl[:, :, -1, c0:c0 + CHUNK] = 0
    y = conv(xh, wh, stride) + (conv(xh, wl, stride) + conv(xl, wh, stride))
    if mutant == 3:                                       # tap (ky = 1, kx = 0) of output column 0: input pixel (row, -1) is the
        S, H, W, C = x.shape                              # pixel in front of (row, 0) in memory -- a zero in the layer function
        flat = x.reshape(S * H * W, C)
        rows = torch.arange(y.shape[1]) * stride          # input row of tap ky = 1
        idx = ((torch.arange(S)[:, None] * H + rows[None, :]) * W - 1)
        add = (flat[idx.clamp(min=0)] @ w[1, 0]) * (idx >= 0)[..., None]
        y = y.clone()
        y[:, :, 0] += add
    return y


def _wino_split_conv(x, w, mutant=None):
    """One 3x3 / stride-1 convolution as Winograd F(2x2,3x3) in split-f16 arithmetic, as a fused device kernel would run it:
    V = B^T d B in fp32 from the decoded hi + lo input, stored as hi/lo pairs (scale 1: |V| <= 4 |d|, the same fp16 range as the
    activations' 4 * value); U = G g G^T in double, rounded once, one power-of-two scale per output channel, hi/lo pairs; the 16
    transform-domain products x_hi u_hi + x_hi u_lo + x_lo u_hi accumulated in fp32 over the input channels; Y = A^T M A in fp32."""
    S, H, W, C = x.shape
    N = w.shape[3]
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1 + 2 * tw - W, 1, 1 + 2 * th - H))
    if mutant == 6:                                       # row H / column W of an odd grid: the next pixels in memory, not zeros
        xn = x.permute(0, 3, 1, 2)
        if H & 1:
            xp[:-1, :, 1 + H, 1:1 + W] = xn[1:, :, 0, :]
        if W & 1:
            xp[:, :, 1:H, 1 + W] = xn[:, :, 1:, 0]
    p = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                   # [S, C, th, tw, 4, 4]
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float32)
    V = torch.einsum("ij,sctujk,lk->sctuil", Bt, p, Bt)                      # fp32 adds of exactly representable inputs
    U = torch.einsum("ij,jkcn,lk->ilcn", G, w.double(), G).float()           # [4, 4, C, N]
    ws = weight_scale(U)
    Vh, Vl = _split(V, 1.0)
    Uh, Ul = _split(U, ws)
    if mutant == 5:
        Vl = Vl.clone()
        Vl[:, MUTANT_CHUNK * CHUNK:(MUTANT_CHUNK + 1) * CHUNK, :, :, 1, 1] = 0
    M = (torch.einsum("sctuil,ilcn->sntuil", Vh, Uh) + (torch.einsum("sctuil,ilcn->sntuil", Vh, Ul) + torch.einsum("sctuil,ilcn->sntuil", Vl, Uh)))
    Y = torch.einsum("ai,sntuil,bl->sntaub", At, M, At)                      # [S, N, th, 2, tw, 2]
    return Y.reshape(S, N, 2 * th, 2 * tw)[:, :, :H, :W].permute(0, 2, 3, 1).contiguous()


# ---- the fp32 mode (BYOLO_PREC_F32): plain fp32 operands, and Winograd F(2x2,3x3) in fp32 as csrc/winograd.hip / wino_fused.hip run it --
MUTANTS_F32 = {1: "one product dropped: input channel 63 at the centre tap",
               2: "the last image column reads zeros for channels 32..63 at one tap",
               3: "left neighbour of column 0 wraps to the pixel before it in memory, for one tap",
               4: "channels 32..63 of x read through their fp16 hi half (split storage leaking into the fp32 mode)",
               5: "Winograd: one of the 16 points dropped for channels 32..63",
               6: "Winograd: the pad row / column of an odd grid takes the neighbouring pixels in memory"}


def _chunk_f32(C):
    """the input channels the fp32 defects touch: 32 .. 63, or all of an input narrower than 64 (the direct small-Cin kernels)"""
    c0 = CHUNK if C >= 2 * CHUNK else 0
    return c0, min(c0 + CHUNK, C)


def _wrap_column0(x, w, y, stride):
    """defect 3 (as _split_conv's): tap (ky = 1, kx = 0) of output column 0 reads the pixel in front of (row, 0) in memory, not a zero"""
    S, H, W, C = x.shape
    flat = x.reshape(S * H * W, C)
    rows = torch.arange(y.shape[1]) * stride              # input row of tap ky = 1
    idx = ((torch.arange(S)[:, None] * H + rows[None, :]) * W - 1)
    add = (flat[idx.clamp(min=0)] @ w[1, 0]) * (idx >= 0)[..., None]
    y = y.clone()
    y[:, :, 0] += add
    return y


def _hi_half(x):
    """defect 4: x with channels 32 .. 63 rounded to the hi half of their split storage"""
    c0, c1 = _chunk_f32(x.shape[3])
    x = x.clone()
    x[..., c0:c1] = _split(x[..., c0:c1], ACT_SCALE)[0]
    return x


def _f32_conv(x, w, stride, mutant=None):
    """The plain fp32 convolution of the fp32 kernels (and of the direct small-Cin kernels in either precision); mutant None is F's."""
    k, C = w.shape[0], x.shape[3]
    c0, c1 = _chunk_f32(C)
    if mutant == 1:
        w = w.clone()
        w[k // 2, k // 2, min(2 * CHUNK - 1, C - 1)] = 0
    if mutant == 4:
        x = _hi_half(x)
    y = conv_nhwc(x, w, stride)
    if mutant == 2:                                       # the centre tap; on stride 2 (even widths, pad on the left) the tap right of it reaches the last column
        kx = k - 1 if stride == 2 else k // 2
        xo, wo = torch.zeros_like(x), torch.zeros_like(w)
        xo[:, :, -1, c0:c1] = x[:, :, -1, c0:c1]
        wo[k // 2, kx, c0:c1] = w[k // 2, kx, c0:c1]
        y = y - conv_nhwc(xo, wo, stride)
    if mutant == 3:
        y = _wrap_column0(x, w, y, stride)
    return y


def _wino_f32_conv(x, w, fused=False, mutant=None):
    """One 3x3 / stride-1 convolution as Winograd F(2x2,3x3) in fp32, as csrc computes it: V = B^T d B in fp32 adds (wino_input_kernel:
    rows, then columns; the pad row / column of an odd grid's last tile are zeros); U = G g G^T in double, rounded once
    (wino_weight_transform); the 16 products accumulated in fp32 over the input channels; Y = A^T M A in fp32 adds -- in
    wino_output_kernel's order (rows left to right, then columns), or with `fused` in wino_fused_kernel's: the transform points
    xi = 0 .. 15 folded one after the other into each of the four outputs."""
    S, H, W, C = x.shape
    N = w.shape[3]
    th, tw = (H + 1) // 2, (W + 1) // 2
    if mutant == 4:
        x = _hi_half(x)
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1 + 2 * tw - W, 1, 1 + 2 * th - H))
    if mutant == 6:                                       # row H / column W of an odd grid: the next pixels in memory, not zeros
        xn = x.permute(0, 3, 1, 2)
        if H & 1:
            xp[:-1, :, 1 + H, 1:1 + W] = xn[1:, :, 0, :]
        if W & 1:
            xp[:, :, 1:H, 1 + W] = xn[:, :, 1:, 0]
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                   # [S, C, th, tw, 4, 4]
    u = torch.stack([d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 2, :] - d[..., 1, :], d[..., 1, :] - d[..., 3, :]], dim=-2)
    V = torch.stack([u[..., 0] - u[..., 2], u[..., 1] + u[..., 2], u[..., 2] - u[..., 1], u[..., 1] - u[..., 3]], dim=-1)
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    U = torch.einsum("ij,jkcn,lk->ilcn", G, w.double(), G).float()           # [4, 4, C, N]
    if mutant == 5:
        c0, c1 = _chunk_f32(C)
        V = V.clone()
        V[:, c0:c1, :, :, 1, 1] = 0
    M = torch.einsum("sctuil,ilcn->ilsntu", V, U)                            # [4, 4, S, N, th, tw]
    if fused:
        At = ((1., 1., 1., 0.), (0., 1., -1., -1.))
        out = []
        for dy in range(2):
            for dx in range(2):
                y = None
                for xi in range(16):
                    c = At[dy][xi >> 2] * At[dx][xi & 3]
                    if c != 0.:
                        y = c * M[xi >> 2, xi & 3] if y is None else y + c * M[xi >> 2, xi & 3]
                out.append(y)
        Y = torch.stack(out, dim=-1).reshape(S, N, th, tw, 2, 2)
    else:
        r = torch.stack([M[0] + M[1] + M[2], M[1] - M[2] - M[3]], dim=0)     # A^T M: [2, 4, S, N, th, tw]
        Y = torch.stack([r[:, 0] + r[:, 1] + r[:, 2], r[:, 1] - r[:, 2] - r[:, 3]], dim=-1).permute(1, 2, 3, 4, 0, 5)      # [S, N, th, tw, dy, dx]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(S, N, 2 * th, 2 * tw)[:, :, :H, :W].permute(0, 2, 3, 1).contiguous()


def gather(sources, dtype):
    """[(NHWC tensor, upsampled)] -> the layer's input: x2 nearest upsample per source, channel concat (exact in every dtype)"""
    parts = []
    for t, up in sources:
        t = t.to(dtype)
        parts.append(t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if up else t)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=3)


def _epilogue(z, a, p, scope, dtype, bn, drop, residual, det):
    """conv output z (and |x| (*) |w| = a, or None) -> [dropout] -> [BN, leaky 0.1] -> [+ residual] | + bias;  returns (y, m)"""
    m = a
    if det:
        b = p[scope + "/conv2d/bias"].to(dtype)
        return z + b, (None if a is None else a + b.abs())
    if drop is not None:                                   # conv -> dropout -> bn -> leaky (layers.py:560-574), TF <= 1.12 form
        seed, ordinal, prob = drop
        keep = rng.keep_mask_torch(seed, ordinal, tuple(z.shape), prob).to(dtype)
        keep_prob = torch.tensor(1.0 - prob, dtype=dtype)
        z = (z / keep_prob) * keep
        m = None if a is None else (a / keep_prob) * keep
    y = z
    if bn:
        g, b, mu, var = (p[scope + "/batch_normalization/" + n].to(dtype) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        inv = g * torch.rsqrt(var + torch.tensor(BN_EPS, dtype=dtype))
        y = (z - mu) * inv + b
        m = None if a is None else m * inv.abs() + (b - mu * inv).abs()
        y = torch.maximum(y, y * 0.1)
    if residual is not None:
        y = y + residual.to(dtype)
        m = None if a is None else m + residual.to(dtype).abs()
    return y, m


def layer_eval(sources, p, scope, k, stride, dtype=torch.float64, bn=True, drop=None, residual=None, det=False):
    """The layer function in `dtype`; p: {name: torch tensor} of the ORIGINAL fp32 parameters.  drop = (seed, ordinal, prob): the mask
    of oracle/rng.py over the layer's whole dropout input [S, h, w, cout] as oracle/cpu_ref.py draws it.  Returns (y, m)."""
    x = gather(sources, dtype)
    w = p[scope + "/conv2d/kernel"].to(dtype)
    assert w.shape[0] == k and w.shape[2] == x.shape[3]
    z = conv_nhwc(x, w, stride)
    a = conv_nhwc(x.abs(), w.abs(), stride)
    return _epilogue(z, a, p, scope, dtype, bn, drop, residual, det)


def layer_f32(sources, p, scope, k, stride, bn=True, drop=None, residual=None, det=False, wino=None, mutant=None):
    """F (wino None; mutant None: layer_eval(dtype=float32) bit for bit) or W (wino 'unfused' | 'fused': the fp32 Winograd path of
    csrc in its kernels' order), then the fp32 epilogue.  mutant: a key of MUTANTS_F32 (see applicable_f32())."""
    x = gather(sources, torch.float32)
    w = p[scope + "/conv2d/kernel"].float()
    if wino:
        assert k == 3 and stride == 1 and wino in ("unfused", "fused")
        z = _wino_f32_conv(x, w, fused=wino == "fused", mutant=mutant)
    else:
        z = _f32_conv(x, w, stride, mutant=mutant)
    return _epilogue(z, None, p, scope, torch.float32, bn, drop, residual, det)[0]


def applicable_f32(k, stride, H, W, wino=None):
    """the fp32 defects that change the arithmetic of such a layer (H, W: the INPUT grid)"""
    if wino:
        return [4, 5] + ([6] if (H & 1) or (W & 1) else [])
    return [1, 2] + ([3] if k == 3 else []) + [4]


def layer_split(sources, p, scope, k, stride, bn=True, drop=None, residual=None, det=False, wino=False, mutant=None, direct=False,
                halves=False):
    """S: the layer in emulated split-f16 arithmetic.  mutant: a key of MUTANTS (see applicable()).  direct: one of the small-Cin
    kernels (csrc/conv_kernels.hip: Cin not a multiple of 32) -- an fp32 convolution of the decoded input with the fp32 weights, the
    output rounded to hi + lo; its defects 1 .. 3 are MUTANTS_F32's, 4 is the residual's hi half as everywhere in this mode.
    halves: the stored pair (hi, lo) itself, in units of the value (tests/_range_plant.py: an element beyond the range has hi = inf)."""
    x = gather(sources, torch.float32)
    w = p[scope + "/conv2d/kernel"].float()
    if direct:
        z = _f32_conv(x, w, stride, mutant=mutant if mutant in (1, 2, 3) else None)
    elif wino:
        assert k == 3 and stride == 1
        z = _wino_split_conv(x, w, mutant=mutant)
    else:
        z = _split_conv(x, w, stride, mutant=mutant)
    if residual is not None and mutant == 4:
        residual = _split(residual.float(), ACT_SCALE)[0]
    y, _ = _epilogue(z, None, p, scope, torch.float32, bn, drop, residual, det)
    if not det:                                            # a detection head's raw output stays fp32
        hi, lo = _split(y, ACT_SCALE)
        if halves:
            return hi, lo
        y = hi + lo
    return y


def applicable(k, stride, H, W, residual=False, det=False, wino=False):
    """the mutants that change the arithmetic of such a layer (H, W: the INPUT grid)"""
    if wino:
        out = [5] + ([6] if (H & 1) or (W & 1) else [])
    else:
        out = [1, 2] + ([3] if k == 3 else [])
    return out + ([4] if residual else [])


def distance(y, y64, m):
    """E = max |y - y64| / m over every element, and where: (E, (sample, y, x, channel))"""
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(y64).all()), "NaN / inf in a layer output"
    assert y.shape == y64.shape, (y.shape, y64.shape)
    r = (y.double() - y64).abs() / m
    i = int(torch.argmax(r))
    import numpy as np
    return float(r.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))


def random_params(shapes, seed):
    """He-scaled kernels, BN statistics around (0, 1): activations of order one through any depth (far inside +-16376 / 4).  beta is
    chosen so that the folded shift beta - mean * gamma * rsqrt(var + eps) has a magnitude in [0.25, 0.75]: the value of a dropped
    element is the shift alone, and below ~0.03 the lo half of such a value is a subnormal fp16 -- the format's absolute floor
    (7.5e-9) would then set the bound of a whole dropout layer instead of its arithmetic."""
    import numpy as np
    g = np.random.default_rng(seed)
    p = {}
    for name, shape in shapes.items():
        if name.endswith("kernel"):
            p[name] = (g.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[:3])))).astype(np.float32)
        elif name.endswith("moving_variance") or name.endswith("gamma"):
            p[name] = (g.random(shape) + 0.5).astype(np.float32)
        else:
            p[name] = (g.standard_normal(shape) * 0.1).astype(np.float32)
    for name in [n for n in shapes if n.endswith("/beta")]:
        s = name[:-len("beta")]
        inv = p[s + "gamma"].astype(np.float64) / np.sqrt(p[s + "moving_variance"].astype(np.float64) + BN_EPS)
        shift = (0.25 + 0.5 * g.random(shapes[name])) * np.where(g.random(shapes[name]) < 0.5, -1.0, 1.0)
        p[name] = (shift + p[s + "moving_mean"].astype(np.float64) * inv).astype(np.float32)
    return p


# ---------------------------------------------------------------------------------------------------------------------------------
# the hand-written graphs of the device test, and their shapes for the CPU test
# ---------------------------------------------------------------------------------------------------------------------------------
BN, DROP = 1, 2
DROP_PROB = 0.25         # exact in every format: keep_prob 0.75, 16-bit threshold 49152
PRIORS = [(0.1, 0.2), (0.3, 0.1), (0.5, 0.5)]


class Graph:
    """Shape and view bookkeeping of one graph (what csrc/byolo_api.hip's builder derives), and -- with `eng` -- the builder calls
    themselves.  A layer is a dict; `view` lists the tensors a reader sees through it: (layer index, upsampled, T-fold tile)."""

    def __init__(self, H, W, B, T=1, eng=None, cls_cnt=2):
        self.H, self.W, self.B, self.T, self.eng, self.cls_cnt = H, W, B, T, eng, cls_cnt
        self.L, self.by_name, self.shapes, self.n_drop = [], {}, {}, 0
        self.first, self.n_backbone_shapes = None, 0       # mark(): index of the first head layer, variables in front of it

    def _push(self, name, idx, **d):
        assert idx is None or idx == len(self.L), (name, idx, len(self.L))
        d.update(idx=len(self.L), name=name)
        self.L.append(d)
        self.by_name[name] = d
        return d

    def _prev(self):
        return self.L[-1] if self.L else dict(H=self.H, W=self.W, C=3, stacked=False, view=[(-1, False, False)])

    def conv(self, name, filters, k=3, stride=1, drop=False, res=None, check=None):
        """check: None, or what the profile must say about this layer's launch (see tests/test_gpu_layer_f64.py)"""
        x = self._prev()
        idx = self.eng.add_conv(name, filters, k, stride, BN | (DROP if drop else 0)) if self.eng else None
        self.shapes[name + "/conv2d/kernel"] = (k, k, x["C"], filters)
        for n in ("gamma", "beta", "moving_mean", "moving_variance"):
            self.shapes[name + "/batch_normalization/" + n] = (filters,)
        d = self._push(name, idx, op="conv", k=k, stride=stride, Cin=x["C"], C=filters, H=x["H"] // stride, W=x["W"] // stride,
                       stacked=x["stacked"], src=x["view"], inH=x["H"], inW=x["W"], drop=None, shortcut=None, check=check, det=False)
        d["view"], d["out"] = [(d["idx"], False, False)], d["idx"]
        if drop:
            d["drop"] = self.n_drop
            self.n_drop += 1
        if res is not None:                                # the add is fused into the convolution's epilogue: the sum is its output
            s = self.by_name[res]
            ridx = self.eng.add_residual(s["idx"]) if self.eng else None
            r = self._push(name + "+", ridx, op="res", C=filters, H=d["H"], W=d["W"], stacked=d["stacked"], conv=d["idx"], shortcut=s["idx"])
            r["view"] = [(r["idx"], False, False)]
            d["shortcut"], d["out"] = s["view"][0][0], r["idx"]
            self.by_name[name] = r
        return d

    def det(self, name, kind, check=None):
        x = self._prev()
        filters = (3 if kind == 0 else 6) * (5 + self.cls_cnt)      # 21 | 42 at two classes
        idx = self.eng.add_detection(name, kind, PRIORS) if self.eng else None
        if self.eng:                                       # the builder's own count (the handle's cls_cnt)
            filters = self.eng.param_shapes()[name + "/conv2d/kernel"][3]
        self.shapes[name + "/conv2d/kernel"] = (1, 1, x["C"], filters)
        self.shapes[name + "/conv2d/bias"] = (filters,)
        d = self._push(name, idx, op="det", k=1, stride=1, Cin=x["C"], C=filters, H=x["H"], W=x["W"], stacked=x["stacked"],
                       src=x["view"], inH=x["H"], inW=x["W"], drop=None, shortcut=None, check=check, det=True)
        d["view"], d["out"] = [(d["idx"], False, False)], d["idx"]
        return d

    def mark(self):
        """byolo_mark_backbone_end: the layers from here on are the head a trainer trains (tests/_head_graphs.py)"""
        if self.eng:
            self.eng.mark_backbone_end()
        self.first, self.n_backbone_shapes = len(self.L), len(self.shapes)

    def up(self, name):
        x = self._prev()
        assert not any(u for _, u, _ in x["view"])
        idx = self.eng.add_upsample() if self.eng else None
        return self._push(name, idx, op="up", C=x["C"], H=2 * x["H"], W=2 * x["W"], stacked=x["stacked"],
                          view=[(i, True, t) for i, _, t in x["view"]])

    def route(self, name, names):
        xs = [self.by_name[n] for n in names]
        idx = self.eng.add_route([x["idx"] for x in xs]) if self.eng else None
        return self._push(name, idx, op="route", C=sum(x["C"] for x in xs), H=xs[0]["H"], W=xs[0]["W"], stacked=xs[0]["stacked"],
                          routes=[x["idx"] for x in xs], view=[v for x in xs for v in x["view"]])

    def stack(self, name, src):
        x = self.by_name[src]
        idx = self.eng.add_stack(x["idx"]) if self.eng else None
        return self._push(name, idx, op="stack", C=x["C"], H=x["H"], W=x["W"], stacked=True, stack_src=x["idx"], view=[(i, u, True) for i, u, _ in x["view"]])

    def topology(self):
        """the graph as oracle/cpu_ref.py's forward() walks it (absolute layer indices)"""
        out = []
        for d in self.L:
            if d["op"] == "conv":
                out.append(dict(op="conv", scope=d["name"], filters=d["C"], k=d["k"], stride=d["stride"], norm="bn" if d["drop"] is None else "dropout_bn"))
            elif d["op"] == "det":
                out.append(dict(op="detection", scope=d["name"], filters=d["C"]))
            elif d["op"] == "res":
                out.append(dict(op="residual", shortcut=d["shortcut"]))
            elif d["op"] == "up":
                out.append(dict(op="upsample"))
            elif d["op"] == "route":
                out.append(dict(op="route", routes=d["routes"]))
            else:
                out.append(dict(op="stack", src=d["stack_src"]))
        return out

    # ---- evaluation of one checked layer ---------------------------------------------------------------------------------
    def samples(self, d):
        return self.B * self.T if d["stacked"] else self.B

    def tensor_shape(self, i):
        d = self.L[i]
        return (self.samples(d), d["H"], d["W"], d["C"])

    def sources(self, d, fetch, seed=None):
        """the layer's sources from fetch(layer index) -> NHWC fp32 tensor: [(tensor, upsampled)]; index -1 is the image (of `seed`)"""
        get = lambda i: fetch(i) if i >= 0 else self.image(seed)
        return [(get(i).repeat_interleave(self.T, dim=0) if t else get(i), u) for i, u, t in d["src"]]

    def image(self, seed):
        """the image batch the device tests feed a case (fp32 in both precisions: the stem kernels read it as it is)"""
        import numpy as np
        return torch.from_numpy(np.random.default_rng(seed).random((self.B, self.H, self.W, 3)).astype(np.float32))

    def direct(self, d):
        """layer d runs on the direct small-Cin kernels (csrc/byolo_api.hip lower(): input channels, or those of the first of two
        sources, not a multiple of 32)"""
        return d["Cin"] % 32 != 0 or (len(d["src"]) == 2 and d["src"][0][0] >= 0 and self.L[d["src"][0][0]]["C"] % 32 != 0)

    def spec(self, d, seed, fetch):
        """keyword arguments of layer_eval / layer_split for layer d"""
        return dict(scope=d["name"], k=d["k"], stride=d["stride"], bn=not d["det"], det=d["det"],
                    drop=None if d["drop"] is None else (seed, d["drop"], DROP_PROB),
                    residual=None if d["shortcut"] is None else fetch(d["shortcut"]))


def stem(g, downs, widen, first=64):
    """the narrow stem: 3 -> 32 at the image's size, `downs` stride-2 layers of 32 (the last one: 64) channels, a 1x1 to `widen`"""
    g.conv("s0", 32)
    for i in range(downs):
        g.conv("s%d" % (i + 1), first if i == downs - 1 else 32, 3, 2)
    return g.conv("w", widen, 1, check=dict(loop="p1", bn=64)) if widen else None


NO_WINO = dict(wino_split=0)
WINO = dict(wino_split=2, wino_split_bn=256, wino_split_min_c=128, wino_split_min_gflop=0.0)
WINO128 = dict(WINO, wino_split_bn=128)


def _a1(g):
    stem(g, 5, 128)
    g.conv("a", 128, check=dict(loop="kx3", bn=64))
    g.conv("b", 256, check=dict(loop="kx3", bn=64))
    g.det("det", 0, check=dict(loop="gen", bn=32))


def _a1_wide(g):                                           # >= 512 tiles of 128 x 128: the planner keeps the 128-wide tile
    g.conv("s0", 32)
    g.conv("a", 256, check=dict(loop="kx3", bn=128))
    g.conv("n", 32, 1)
    g.det("det", 0)


def _a2(g):
    stem(g, 5, 128)
    g.conv("a", 256, check=dict(loop="kx3", bn=256))
    g.conv("b", 512, check=dict(loop="kx3", bn=256))
    g.det("det", 1, check=dict(loop="p1", bn=64))


def _a3(g):
    stem(g, 5, 128)
    g.conv("a", 128, check=dict(loop="kx3", bn=64))
    g.det("det", 0, check=dict(loop="gen", bn=32))


def _a4(g):
    stem(g, 5, 128)
    g.conv("a", 128, res="w", check=dict(loop="kx3", bn=64))
    g.conv("b", 128, drop=True, check=dict(loop="kx3", bn=64))
    g.conv("c", 128, drop=True, res="a", check=dict(loop="kx3", bn=64))
    g.det("det", 0, check=dict(loop="gen", bn=32))


def _b1(g):
    stem(g, 5, 256)
    g.conv("p", 128, 1, check=dict(loop="p1", bn=64))
    g.conv("q", 512, 1, check=dict(loop="p1", bn=64))
    g.conv("r", 64, 1, drop=True, check=dict(loop="p1", bn=64))
    g.det("det", 1, check=dict(loop="p1", bn=64))


def _b2(g):                                                # (the builder takes stride 2 on even grids only: 12 x 20 -> 6 x 10 -> 3 x 5)
    stem(g, 4, 128)
    g.conv("d", 256, 3, 2, check=dict(loop="gen", bn=64))
    g.conv("e", 128, 3, 2, check=dict(loop="gen", bn=64))
    g.up("up")
    g.route("cat", ["up", "d"])                            # 128 (x2 upsampled) + 256 plain channels: the K range crosses the sources
    g.conv("f", 128, 1, check=dict(loop="gen", bn=64))
    g.det("det", 0, check=dict(loop="gen", bn=32))


def _b2_odd(g):                                            # 10 x 14 -> 5 x 7
    stem(g, 4, 128)
    g.conv("d", 256, 3, 2, check=dict(loop="gen", bn=64))
    g.det("det", 1, check=dict(loop="p1", bn=64))


def _c1(cin, cout):
    def build(g):
        stem(g, 5, cin)
        g.conv("a", cout, check=dict(wino=256))
        g.det("det", 1, check=dict(loop="p1", bn=64))
    return build


def _c2(g):
    stem(g, 5, 256)
    g.conv("a", 384, check=dict(wino=128))
    g.conv("m", 256, 1, check=dict(loop="p1", bn=64))
    g.conv("b", 128, check=dict(wino=128))
    g.det("det", 0, check=dict(loop="gen", bn=32))


def _c3(g):
    stem(g, 5, 256)
    g.conv("a", 256, check=dict(wino=256, chunks=3))
    g.det("det", 1, check=dict(loop="p1", bn=64))


def _c4(g):
    stem(g, 5, 256)
    g.conv("a", 256, res="w", check=dict(wino=256))        # epilogue_res
    g.conv("b", 256, drop=True, check=dict(wino=256))
    g.conv("c", 256, drop=True, res="a", check=dict(loop="kx3", bn=64))      # (the Winograd residual epilogue carries no dropout: direct)
    g.det("det", 1, check=dict(loop="p1", bn=64))


def _c5(g):
    stem(g, 5, 128)
    g.conv("a", 128, check=dict(wino=128, fallback=dict(loop="kx3", bn=64)))      # (128 output channels: the 128-channel form whatever wino_split_bn asks)
    g.det("det", 0, check=dict(loop="gen", bn=32))


def _d2(wino):
    def build(g):
        stem(g, 5, 128)
        g.stack("st", "w")
        g.conv("r", 128, drop=True, check=dict(loop="kx3", bn=64))          # every source a T-fold tile: once per image, T masked epilogues
        g.conv("t", 128, drop=True, check=dict(wino=128) if wino else dict(loop="kx3", bn=64))
        g.det("det", 2, check=dict(loop="p1", bn=64))
    return build


def _sk(g):
    """Widths at which EVERY loop is admissible for stream-K (csrc/conv_igemm.hip conv_plan_split: tiles * K-tiles beyond the grid of
    min(512, that product) rounded down to 8 -- a product that is a multiple of 8 below 512 leaves no unit to share): 3 row tiles of
    the 6 x 10 x 5 grid, 64 / 96 / 160 / 192 channels.  Also: 192 and 96 output channels in 128-wide tiles (columns past Cout)."""
    stem(g, 4, 128)
    g.conv("d", 64, 3, 2, check=dict(loop="gen", bn=64, sk=True))          # 12 x 20 -> 6 x 10
    g.conv("a", 192, check=dict(loop="kx3", bn=128, sk=True))
    g.conv("p", 96, 1, check=dict(loop="p1", bn=128, sk=True))
    g.conv("e", 64, 3, 2, check=dict(loop="gen", bn=64, sk=True))          # -> 3 x 5: ONE partial row tile
    g.up("up")
    g.route("cat", ["up", "p"])
    g.conv("f", 128, 1, check=dict(loop="gen", bn=64, sk=True))
    g.det("det", 0, check=dict(loop="gen", bn=32, sk=True))


# the fused paths (tests/test_gpu_layer_f64.py builds each of these twice)
def _fused_a2(follower):
    def build(g):
        stem(g, 5, 128)
        g.conv("a", 256, check=dict(loop="kx3", bn=64))    # 256 output channels + ONE reader: a back-to-back pair under b2b = 2
        if follower:
            g.conv("f", 128, 1, check=dict(loop="p1", bn=64))
            g.conv("b", 128, check=dict(loop="kx3", bn=64))
        g.det("det", 1, check=dict(loop="p1", bn=64))
    return build


def _fed(g):
    """a small stacked head: a replayed 1x1 (STEP_REP) and a 1x1 over [upsampled, T-fold tile] (partial sums + finish), each read by
    ONE Winograd convolution -- what byolo_plan_opts.wino_split_feed folds into that convolution's input transform"""
    stem(g, 4, 128)
    g.conv("lo", 128, 3, 2)                                # 12 x 20 -> 6 x 10, per image
    g.stack("st", "lo")
    g.conv("r", 128, 1, drop=True, check=dict(loop="p1", bn=64))
    g.conv("t", 128, drop=True, check=dict(wino=128))
    g.conv("u", 128, 1, check=dict(loop="p1", bn=64))
    g.up("up")
    g.stack("sk", "w")
    g.route("cat", ["up", "sk"])
    g.conv("f", 128, 1, drop=True, check=dict(multi=True))      # several launches: the per-image half, the low-resolution half, the finish
    g.conv("v", 128, check=dict(wino=128))
    g.det("det", 2, check=dict(loop="p1", bn=64))


def _grid(gh, gw, downs=5):
    return gh << downs, gw << downs


# name -> (image H, W, B, T, plan options, graph)
CASES = {}
for _n, (_gh, _gw, _b) in {"5x7x11": (5, 7, 11), "6x10x5": (6, 10, 5)}.items():
    CASES["A1 kx3 128x64 " + _n] = _grid(_gh, _gw) + (_b, 1, NO_WINO, _a1)
    CASES["B3 kx3 ksplit=3 " + _n] = _grid(_gh, _gw) + (_b, 1, dict(NO_WINO, ksplit=3), _a1)
CASES["A1 kx3 128x128 64x96x8"] = (64, 96, 8, 1, NO_WINO, _a1_wide)
CASES["A2 kx3 128x256 3x5x20"] = _grid(3, 5) + (20, 1, dict(NO_WINO, kx3_wide=2), _a2)
for _gh, _gw in ((1, 3), (3, 1), (2, 2)):
    CASES["A3 kx3 %dx%dx9" % (_gh, _gw)] = _grid(_gh, _gw) + (9, 1, NO_WINO, _a3)
    CASES["C5 wino %dx%dx9" % (_gh, _gw)] = _grid(_gh, _gw) + (9, 1, WINO, _c5)
CASES["A4 kx3 epilogues 5x7x11"] = _grid(5, 7) + (11, 1, NO_WINO, _a4)
CASES["B1 p1 5x7x11"] = _grid(5, 7) + (11, 1, NO_WINO, _b1)
CASES["B3 p1 ksplit=3 5x7x11"] = _grid(5, 7) + (11, 1, dict(NO_WINO, ksplit=3), _b1)
CASES["B2 general 12x20x7"] = _grid(12, 20, 4) + (7, 1, NO_WINO, _b2)
CASES["B3 general ksplit=3 12x20x7"] = _grid(12, 20, 4) + (7, 1, dict(NO_WINO, ksplit=3), _b2)
CASES["B3 every loop streamk=2 6x10x5"] = _grid(12, 20, 4) + (5, 1, dict(NO_WINO, streamk=2), _sk)
CASES["B3 every loop ksplit=3 6x10x5"] = _grid(12, 20, 4) + (5, 1, dict(NO_WINO, ksplit=3), _sk)
CASES["B2 general 10x14x7"] = _grid(10, 14, 4) + (7, 1, NO_WINO, _b2_odd)
CASES["C1 wino<256> 256->256 3x5x23"] = _grid(3, 5) + (23, 1, WINO, _c1(256, 256))
CASES["C1 wino<256> 512->512 5x7x3"] = _grid(5, 7) + (3, 1, WINO, _c1(512, 512))
CASES["C1 wino<256> 128->256 6x10x5"] = _grid(6, 10) + (5, 1, WINO, _c1(128, 256))
CASES["C2 wino<128> 3x5x23"] = _grid(3, 5) + (23, 1, WINO128, _c2)
CASES["C3 wino chunks 5x7x11"] = _grid(5, 7) + (11, 1, dict(WINO, wino_split_chunk_mb=0.8), _c3)      # 11 samples of 196 608 V bytes: 4 + 4 + 3
CASES["C4 wino epilogues 3x5x23"] = _grid(3, 5) + (23, 1, WINO, _c4)
CASES["D2 stacked T=3 5x7x4"] = _grid(5, 7) + (4, 3, NO_WINO, _d2(False))
CASES["D2 stacked T=3 wino 5x7x4"] = _grid(5, 7) + (4, 3, WINO, _d2(True))
CASES["E b2b 3x3(256) -> detection 3x5x20"] = _grid(3, 5) + (20, 1, dict(NO_WINO, b2b=2), _fused_a2(False))
CASES["E b2b 3x3(256) -> 1x1(128) 3x5x20"] = _grid(3, 5) + (20, 1, dict(NO_WINO, b2b=2), _fused_a2(True))
for _feed in (1, 2, 3):
    CASES["E wino feed %d 6x10x3 T=3" % _feed] = _grid(12, 20, 4) + (3, 3, dict(WINO, wino_split_feed=_feed, wino_split_chunk_mb=0.3), _fed)


# ---------------------------------------------------------------------------------------------------------------------------------
# The direct small-Cin kernels (csrc/conv_kernels.hip: conv_stem3x3_kernel, conv_direct_kernel), which serve BOTH precisions: the
# shapes of tests/test_gpu_layers.py::test_general_direct_convolution_and_view_shortcuts behind the narrow stem, so that they meet
# odd grids.  `v`: the variants both tables' tests want of the layer's launches, in order (-1: the direct kernels).
# ---------------------------------------------------------------------------------------------------------------------------------
DIRECT = dict(v=[-1])


def _direct(g):
    g.conv("s0", 32, check=DIRECT)                         # the 3 -> 32 stem (conv_stem3x3_kernel), on the image itself
    for i in range(4):
        g.conv("s%d" % (i + 1), 64 if i == 3 else 32, 3, 2)      # -> 10 x 14 | 12 x 20
    g.conv("n", 24, 1)
    g.conv("h", 40, check=DIRECT)                          # Cin = 24, stride 1: 9 * 24 * 40 weights (34 KB) sit in LDS
    g.route("rn", ["n"])                                   # (an identity view: b reads n)
    g.conv("b", 40, 3, 2, drop=True, check=DIRECT)         # Cin = 24 at stride 2 -> 5 x 7 | 6 x 10
    g.conv("c", 40, res="b", check=DIRECT)                 # Cin = 40 at stride 1 with a residual; 9 * 40 * 40 weights (58 KB): not in LDS
    g.conv("d", 256, check=DIRECT)                         # 9 * 40 * 256 weights (369 KB): not in LDS
    g.up("up")
    g.route("cat", ["up", "h"])                            # [256 upsampled, 40 plain] = 296 channels
    g.conv("e", 20, 1, check=DIRECT)                       # 20 output channels (the 8-channel groups end inside the third)
    g.det("det", 0, check=DIRECT)                          # a detection head over 20 channels


CASES["K direct small-Cin 5x7x3"] = _grid(10, 14, 4) + (3, 1, NO_WINO, _direct)
CASES["K direct small-Cin 6x10x2"] = _grid(12, 20, 4) + (2, 1, NO_WINO, _direct)


# ---------------------------------------------------------------------------------------------------------------------------------
# The fp32 mode (tests/test_gpu_layer_f64_fp32.py, tests/test_layer_ref_f32_cpu.py).  check = dict(v = the variants of the layer's
# launches in the profile, in order (include/byolo.h: 128 / 64 / 32 conv_igemm_kernel by tile width, -1 direct, -2 / -3 the Winograd
# transforms, 129 the row-streaming Winograd-domain GEMM, 130 wino_fused_kernel, 131 / 132 a row-streaming 1x1, -5
# finish_upsampled_kernel) [, wino = 'unfused' | 'fused': W is the unit's other half] [, ks = 'ksplit' | 'sk': the GEMM launch runs in
# K slices / on a stream-K grid] [, chunked: the last Winograd chunk is shorter] [, deep: a slot of the fused kernel gets several row
# tiles]).  Tile widths as byolo_plan.hip picks them in this mode: cout <= 32 -> 32, <= 64 -> 64, beyond -> 128, but 64 where cout is
# a multiple of 128 and the launch has fewer than 512 tiles of 128 x 128 -- every launch of these grids except the 64 x 96 x 8 one.
# ---------------------------------------------------------------------------------------------------------------------------------
def V(*v, **kw):
    return dict(v=list(v), **kw)


ONE_PASS = dict(ksplit=0, streamk=0)                                          # whole tiles in one pass (the cost model gives launches this small a stream-K grid)
SK = dict(ksplit=-1, streamk=2)                                               # stream-K wherever admissible (it needs the K-slice knob on its default)
IG = dict(ONE_PASS, winograd=0, stream1x1=0)                                  # conv_igemm_kernel for everything
WU = dict(ONE_PASS, winograd=2, wino_fused=0, gemm_stream=0, stream1x1=0)     # -2, the GEMM on conv_igemm_kernel over 16 * P_pad rows, -3
WS = dict(ONE_PASS, winograd=2, wino_fused=0, gemm_stream=1, stream1x1=0)     # -2, the row-streaming GEMM (129), -3
WF = dict(ONE_PASS, winograd=2, wino_fused=2, stream1x1=0)                    # -2, wino_fused_kernel (130)
ST = dict(ONE_PASS, winograd=0, stream1x1=2)                                  # 131 / 132 for every 1x1 gemm_stream_kernel can express
WINO_V = {"gemm": (-2, 128, -3), "stream": (-2, 129, -3), "fused": (-2, 130)}      # (the Winograd-domain GEMM keeps the 128-wide tile)


def W(how, chunks=1, **kw):
    return dict(v=list(WINO_V[how]) * chunks, wino="fused" if how == "fused" else "unfused", **kw)


def stem_f32(g, downs, widen, v):
    g.conv("s0", 32)
    for i in range(downs):
        g.conv("s%d" % (i + 1), 64 if i == downs - 1 else 32, 3, 2)
    return g.conv("w", widen, 1, check=V(v))


def _f_a1(ks=None):
    def build(g):
        stem_f32(g, 5, 128, 64)
        g.conv("a", 128, check=V(64, ks=ks))
        g.conv("b", 256, check=V(64, ks=ks))
        g.det("det", 0, check=V(32, ks=ks))               # 21 channels: the 128 x 32 tile
    return build


def _f_wide(ks=None):
    def build(g):                                          # 384 row tiles x 2: the planner keeps the 128-wide tile
        g.conv("s0", 32)
        g.conv("a", 256, check=V(128, ks=ks))
        g.conv("n", 32, 1)
        g.det("det", 0)
    return build


def _f_a3(g):
    stem_f32(g, 5, 128, 64)
    g.conv("a", 128, check=V(64))
    g.det("det", 0, check=V(32))


def _f_sk(ks):
    """_sk's widths: admissible for stream-K on the fp32 tiles as well (tiles * K-tiles: d 3 * 36, a 6 * 18, p 3 * 6, e 1 * 27,
    f 6 * 5, det 3 * 4 -- none a multiple of 8 below 512).  192 and 96 output channels: 128-wide tiles with columns past cout."""
    def build(g):
        stem_f32(g, 4, 128, 64)
        g.conv("d", 64, 3, 2, check=V(64, ks=ks))          # 12 x 20 -> 6 x 10
        g.conv("a", 192, check=V(128, ks=ks))
        g.conv("p", 96, 1, check=V(128, ks=ks))
        g.conv("e", 64, 3, 2, check=V(64, ks=ks))          # -> 3 x 5: ONE partial row tile
        g.up("up")
        g.route("cat", ["up", "p"])
        g.conv("f", 128, 1, check=V(64, ks=ks))
        g.det("det", 0, check=V(32, ks=ks))
    return build


def _f_b2(ks=None):
    def build(g):                                          # 12 x 20 -> 6 x 10 -> 3 x 5
        stem_f32(g, 4, 128, 64)
        g.conv("d", 256, 3, 2, check=V(64, ks=ks))
        g.conv("e", 128, 3, 2, check=V(64, ks=ks))
        g.up("up")
        g.route("cat", ["up", "d"])                        # 128 (x2 upsampled) + 256 plain channels: the K range crosses the sources
        g.conv("f", 128, 1, check=V(64, ks=ks))
        g.det("det", 0, check=V(32, ks=ks))
    return build


def _f_b2_odd(g):                                          # 10 x 14 -> 5 x 7
    stem_f32(g, 4, 128, 64)
    g.conv("d", 256, 3, 2, check=V(64))
    g.det("det", 1, check=V(64))                           # 42 channels: the 128 x 64 tile


def _f_low(lowmain):
    """the concat of a stacked head, [upsampled stacked tensor, T-fold tile]: the tile's half once per image (STEP_PARTIAL), then --
    lowmain on -- the stacked half at ITS resolution and finish_upsampled_kernel (-5), or -- off -- a STEP_MAIN launch at the output's"""
    def build(g):
        stem_f32(g, 4, 128, 64)
        g.conv("lo", 128, 3, 2)                            # 12 x 20 -> 6 x 10, per image
        g.stack("st", "lo")
        g.conv("r", 128, 1, drop=True, check=V(64))        # the replayed 1x1 (STEP_REP)
        g.up("up")
        g.stack("sk", "w")
        g.route("cat", ["up", "sk"])
        g.conv("f", 128, 1, drop=True, check=V(64, 64, -5) if lowmain else V(64, 64))
        g.det("det", 2, check=V(64))
    return build


def _f_a4(how):
    def build(g):                                          # residual | dropout | dropout with residual | detection bias
        stem_f32(g, 5, 128, 64)
        mk = (lambda: W(how)) if how else (lambda: V(64))
        g.conv("a", 128, res="w", check=mk())
        g.conv("b", 128, drop=True, check=mk())
        g.conv("c", 128, drop=True, res="a", check=mk())
        g.det("det", 0, check=V(32))
    return build


def _f_d(g):
    """stacked, T = 3: the replayed 1x1 (every source a T-fold tile: once per image, T masked epilogues), and the convolution over
    [stacked tensor, T-fold tile] -- the tile's half once per image, picked up as an addend by the STEP_MAIN launch -- without and
    with a fused residual"""
    stem_f32(g, 5, 128, 64)
    g.stack("st", "w")
    g.conv("r", 128, 1, drop=True, check=V(64))
    g.route("cat1", ["r", "st"])
    g.conv("c", 128, check=V(64, 64))
    g.route("cat2", ["c", "st"])
    g.conv("c2", 128, res="r", check=V(64, 64))
    g.det("det", 2, check=V(64))


def _f_w1(cin, cout, how, chunks=1, ks=None):
    def build(g):
        stem_f32(g, 5, cin, 64)
        g.conv("a", cout, check=W(how, chunks, ks=ks, chunked=chunks > 1))
        g.det("det", 1, check=V(64))
    return build


def _f_w3(g):                                              # 100 output channels: a multiple of 4, not of 64 (columns 100 .. 127 of the tile do not exist)
    stem_f32(g, 5, 128, 64)
    g.conv("a", 100, check=W("gemm"))
    g.det("det", 0, check=V(-1))                           # (100 input channels: the direct kernel)


def _f_fused(g):                                           # 1, 2, 4 and 8 column tiles of 64 channels
    stem_f32(g, 5, 64, 64)
    g.conv("a", 64, check=W("fused"))
    g.conv("b", 128, check=W("fused"))
    g.conv("c", 256, check=W("fused"))
    g.conv("d", 512, check=W("fused"))
    g.det("det", 1, check=V(64))


def _f_deep(g):
    """140 samples of 6 x 10 output tiles: 66 row tiles on the 64 slots of 8 column tiles -- two slots run two row tiles.  (The samples
    come from a stack of T = 35: the stem runs on 4 images.)"""
    stem_f32(g, 4, 64, 64)
    g.stack("st", "w")
    g.conv("r", 64, 1)                                     # (no dropout: not replayed -- a stacked tensor of its own)
    g.conv("a", 512, check=W("fused", deep=True))
    g.conv("n", 64, 1)
    g.det("det", 2)


def _f_stream(kind, v_det):
    def build(g):
        stem_f32(g, 5, 64, 132)                            # C = 64, N = 64: the 64-wide tile
        g.conv("p", 128, 1, check=V(131))                  # C = 64
        g.conv("q", 256, 1, check=V(131))                  # C = 128
        g.conv("u", 512, 1, check=V(131))
        g.conv("r", 64, 1, drop=True, check=V(132))        # C = 512, dropout
        g.det("det", kind, check=V(v_det))
    return build


def _f_stream_main(g):
    stem_f32(g, 5, 128, 131)
    g.stack("st", "w")
    g.conv("r", 128, 1, drop=True, check=V(64))            # (STEP_REP: conv_igemm_kernel)
    g.route("cat", ["r", "st"])
    g.conv("f", 128, 1, drop=True, check=V(64, 131))       # the tile's half once per image, then STEP_MAIN with that addend, streaming
    g.det("det", 2, check=V(132))


def _f_inj(inject):
    """what an injected-mask call changes: no Winograd, no row-streaming launch, no 128-wide tile"""
    def build(g):
        stem_f32(g, 5, 128, 64 if inject else 131)
        g.conv("a", 192, drop=True, check=V(64) if inject else W("gemm"))        # (192: no whole column tiles for 129 / 130)
        g.conv("p", 128, 1, drop=True, check=V(64) if inject else V(131))
        g.conv("c", 128, drop=True, res="p", check=V(64) if inject else W("fused"))
        g.det("det", 0, check=V(32))                       # (21 channels pad to 32 columns: gemm_stream_kernel's 64-wide tile does not take them)
    return build


# name -> (image H, W, B, T, plan options, graph);  INJECT_F32: the cases that hand byolo_forward the masks of oracle/rng.py
CASES_F32, INJECT_F32 = {}, set()
for _n, (_gh, _gw, _b) in {"5x7x11": (5, 7, 11), "6x10x5": (6, 10, 5)}.items():
    CASES_F32["I1 igemm 128x64 + 128x32 " + _n] = _grid(_gh, _gw) + (_b, 1, IG, _f_a1())
    CASES_F32["I3 igemm ksplit=3 " + _n] = _grid(_gh, _gw) + (_b, 1, dict(IG, ksplit=3), _f_a1("ksplit"))
CASES_F32["I1 igemm 128x128 64x96x8"] = (64, 96, 8, 1, IG, _f_wide())
CASES_F32["I3 igemm 128x128 ksplit=3 64x96x8"] = (64, 96, 8, 1, dict(IG, ksplit=3), _f_wide("ksplit"))
CASES_F32["I3 igemm 128x128 streamk=2 64x96x8"] = (64, 96, 8, 1, dict(IG, **SK), _f_wide("sk"))
for _gh, _gw in ((1, 3), (3, 1), (2, 2)):
    CASES_F32["I2 igemm %dx%dx9" % (_gh, _gw)] = _grid(_gh, _gw) + (9, 1, IG, _f_a3)
    CASES_F32["W1 wino gemm %dx%dx9" % (_gh, _gw)] = _grid(_gh, _gw) + (9, 1, WU, _f_w1(128, 128, "gemm"))
    CASES_F32["W1 wino stream %dx%dx9" % (_gh, _gw)] = _grid(_gh, _gw) + (9, 1, WS, _f_w1(128, 128, "stream"))
CASES_F32["I3 every loop streamk=2 6x10x5"] = _grid(12, 20, 4) + (5, 1, dict(IG, **SK), _f_sk("sk"))
CASES_F32["I3 every loop ksplit=3 6x10x5"] = _grid(12, 20, 4) + (5, 1, dict(IG, ksplit=3), _f_sk("ksplit"))
CASES_F32["G1 general 12x20x7"] = _grid(12, 20, 4) + (7, 1, IG, _f_b2())
CASES_F32["G1 general ksplit=3 12x20x7"] = _grid(12, 20, 4) + (7, 1, dict(IG, ksplit=3), _f_b2("ksplit"))
CASES_F32["G1 general 10x14x7"] = _grid(10, 14, 4) + (7, 1, IG, _f_b2_odd)
CASES_F32["G2 stacked concat lowmain=1 12x20x3 T=3"] = _grid(12, 20, 4) + (3, 3, dict(IG, lowmain=1), _f_low(True))
CASES_F32["G2 stacked concat lowmain=0 12x20x3 T=3"] = _grid(12, 20, 4) + (3, 3, dict(IG, lowmain=0), _f_low(False))
CASES_F32["P1 epilogues igemm 5x7x11"] = _grid(5, 7) + (11, 1, IG, _f_a4(None))
CASES_F32["P1 epilogues wino gemm 5x7x11"] = _grid(5, 7) + (11, 1, WU, _f_a4("gemm"))
CASES_F32["P1 epilogues wino stream 5x7x11"] = _grid(5, 7) + (11, 1, WS, _f_a4("stream"))
CASES_F32["P1 epilogues wino fused 5x7x11"] = _grid(5, 7) + (11, 1, WF, _f_a4("fused"))
CASES_F32["D1 stacked T=3 5x7x4"] = _grid(5, 7) + (4, 3, IG, _f_d)
for _how, _o in (("gemm", WU), ("stream", WS)):
    CASES_F32["W1 wino %s 256->256 3x5x23" % _how] = _grid(3, 5) + (23, 1, _o, _f_w1(256, 256, _how))      # P = 138: P_pad 256
    CASES_F32["W1 wino %s 128->256 5x7x3" % _how] = _grid(5, 7) + (3, 1, _o, _f_w1(128, 256, _how))
    CASES_F32["W1 wino %s 128->128 6x10x5" % _how] = _grid(6, 10) + (5, 1, _o, _f_w1(128, 128, _how))
    # 11 samples of 16 * 12 * (256 + 256) * 4 = 393 216 V + M bytes against 1.3 MB: 4 equal chunks of 3 -- 3 + 3 + 3 + 2
    CASES_F32["W2 wino %s chunks 5x7x11" % _how] = _grid(5, 7) + (11, 1, dict(_o, wino_chunk_mb=1.3), _f_w1(256, 256, _how, chunks=4))
CASES_F32["W3 wino gemm 100 channels 5x7x3"] = _grid(5, 7) + (3, 1, WU, _f_w3)
CASES_F32["W4 wino gemm ksplit=3 256->256 5x7x3"] = _grid(5, 7) + (3, 1, dict(WU, ksplit=3), _f_w1(256, 256, "gemm", ks="ksplit"))      # 8 K-tiles
CASES_F32["F1 fused N = 64 .. 512 5x7x11"] = _grid(5, 7) + (11, 1, WF, _f_fused)           # 2 row tiles on 512 .. 64 slots
CASES_F32["F1 fused N = 64 .. 512 6x10x5"] = _grid(6, 10) + (5, 1, WF, _f_fused)
CASES_F32["F2 fused 66 row tiles on 64 slots 12x20x4 T=35"] = _grid(12, 20, 4) + (4, 35, WF, _f_deep)
# 16 * 12 * 128 * 4 = 98 304 V bytes per sample against 0.4 MB: chunks of 4 -- 4 + 4 + 3
CASES_F32["F3 fused chunks 5x7x11"] = _grid(5, 7) + (11, 1, dict(WF, wino_chunk_mb=0.4), _f_w1(128, 128, "fused", chunks=3))
CASES_F32["S1 stream 1x1 5x7x11"] = _grid(5, 7) + (11, 1, ST, _f_stream(1, 132))           # 385 rows: the fourth row tile holds ONE row
# the 21-channel head pads to 32 columns (the 128 x 32 tile); gemm_stream_kernel's narrowest tile is 64 wide and byolo_plan.hip takes
# a head for it only when it pads to exactly that -- so this head stays on conv_igemm_kernel under stream1x1 = 2 as well
CASES_F32["S1 stream 1x1 6x10x5"] = _grid(6, 10) + (5, 1, ST, _f_stream(0, 32))
CASES_F32["S2 stream STEP_MAIN 5x7x4 T=3"] = _grid(5, 7) + (4, 3, ST, _f_stream_main)
CASES_F32["J0 hashed masks 5x7x11"] = _grid(5, 7) + (11, 1, dict(winograd=2, wino_fused=2, gemm_stream=0, stream1x1=2), _f_inj(False))
CASES_F32["J1 injected masks 5x7x11"] = _grid(5, 7) + (11, 1, dict(winograd=2, wino_fused=2, gemm_stream=0, stream1x1=2), _f_inj(True))
INJECT_F32.add("J1 injected masks 5x7x11")
for _n in ("K direct small-Cin 5x7x3", "K direct small-Cin 6x10x2"):
    CASES_F32[_n] = CASES[_n][:4] + (IG, _direct)


def case_seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def checked(g):
    return [d for d in g.L if d.get("check") is not None]


def measure(g, d, p, seed, fetch, y_dev=None, mutants=False, precision="split"):
    """{E, S, F} of layer d on the input fetch() hands out -- and E of every applicable mutant of S: E = max |y - y64| / m.
    precision 'f32': {E, F, W} (W on a Winograd layer only: check['wino'] = 'unfused' | 'fused') and the mutants of F or W.
    'unit' is the unit of the device bound: max(S, F) | max(W, F) | F."""
    src = g.sources(d, fetch, seed)
    kw = g.spec(d, seed, fetch)
    y64, m = layer_eval(src, p, dtype=torch.float64, **kw)
    if precision == "f32":
        wino = d["check"].get("wino")
        out = dict(F=distance(layer_eval(src, p, dtype=torch.float32, **kw)[0], y64, m)[0])
        if wino:
            out["W"] = distance(layer_f32(src, p, wino=wino, **kw), y64, m)[0]
        out["unit"] = max(out["F"], out.get("W", 0.0))
        if y_dev is not None:
            out["E"], out["worst"] = distance(y_dev, y64, m)
        if mutants:
            for k in applicable_f32(d["k"], d["stride"], d["inH"], d["inW"], wino=wino):
                out["mutant %d" % k] = distance(layer_f32(src, p, wino=wino, mutant=k, **kw), y64, m)[0]
        return out
    wino = "wino" in d["check"]
    direct = dict(direct=True) if g.direct(d) else {}
    out = dict(F=distance(layer_eval(src, p, dtype=torch.float32, **kw)[0], y64, m)[0],
               S=distance(layer_split(src, p, wino=wino, **direct, **kw), y64, m)[0])
    out["unit"] = max(out["S"], out["F"])
    if y_dev is not None:
        out["E"], out["worst"] = distance(y_dev, y64, m)
    if mutants:
        for k in applicable(d["k"], d["stride"], d["inH"], d["inW"], residual=kw["residual"] is not None, det=d["det"], wino=wino):
            out["mutant %d" % k] = distance(layer_split(src, p, wino=wino, mutant=k, **direct, **kw), y64, m)[0]
    return out
