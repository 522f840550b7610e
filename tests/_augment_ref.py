"""float32 restatement of csrc/augment.hip (byolo_augment_batch), operation for operation, in numpy: the crop, TF1's legacy
bilinear resize, the flip, the box blur, TF's AdjustSaturation / AdjustHue CPU kernels, brightness and the three noise ops with
the kernel's counter-based hash.  Everything is bit-identical to the kernel except the Gaussian term, whose logf / cosf are
numpy's (the tests allow 1e-6 absolute there).  Plans are records of byolo.augment.PLAN_DTYPE (or anything indexable by field)."""
import numpy as np

f32 = np.float32
K255 = f32(1.0) / f32(255.0)
P_SALT, P_PEPPER, P_GAUSS_1, P_GAUSS_2 = 1, 2, 3, 4
M32 = 0xFFFFFFFF


def mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x21F0AAAD)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x735A2D97)
    x ^= x >> np.uint32(15)
    return x


def aug_hash(key, n, purpose):
    key = int(key)
    n = np.asarray(n, dtype=np.uint32)
    x = mix32(n + np.uint32(key & M32))
    x ^= np.uint32(((key >> 32) + purpose * 0x9E3779B9) & M32)
    return mix32(x)


def uniform(key, n, purpose):
    return (aug_hash(key, n, purpose) >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)


def gaussian(key, n):
    u1 = f32(1.0) - uniform(key, n, P_GAUSS_1)
    u2 = uniform(key, n, P_GAUSS_2)
    return np.sqrt(f32(-2.0) * np.log(u1)) * np.cos(f32(6.2831855) * u2)


# ---- colour ---------------------------------------------------------------------------------------------------------------
def adjust_saturation(rgb, factor):
    """TF adjust_saturation_op.cc (CPU) on [..., 3] float32."""
    rgb = np.asarray(rgb, dtype=f32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        vv = np.maximum(r, np.maximum(g, b))
        rng = vv - np.minimum(r, np.minimum(g, b))
        s = np.where(vv > 0, rng / vv, f32(0)).astype(f32)
        norm = f32(1.0) / (f32(6.0) * rng)
        h_r = norm * (g - b)
        h_g = ((norm * (b - r)).astype(np.float64) + 2.0 / 6.0).astype(f32)
        h_b = ((norm * (r - g)).astype(np.float64) + 4.0 / 6.0).astype(f32)
    hh = np.where(r == vv, h_r, np.where(g == vv, h_g, h_b)).astype(f32)
    hh = np.where(rng <= 0, f32(0), hh)
    hh = np.where(hh < 0, hh + f32(1.0), hh).astype(f32)
    s = np.minimum(f32(1.0), np.maximum(f32(0.0), s * f32(factor)))
    c = s * vv
    m = vv - c
    dh = hh * f32(6.0)
    cat = dh.astype(np.int32)
    fm = dh.copy()
    while (fm <= 0).any():
        fm = np.where(fm <= 0, fm + f32(2.0), fm)
    while (fm >= 2).any():
        fm = np.where(fm >= 2, fm - f32(2.0), fm)
    x = c * (f32(1.0) - np.abs(fm - f32(1.0)))
    z = np.zeros_like(c)
    tab = {0: (c, x, z), 1: (x, c, z), 2: (z, c, x), 3: (z, x, c), 4: (x, z, c), 5: (c, z, x)}
    out = np.zeros(rgb.shape, dtype=f32)
    for k, (rr, gg, bb) in tab.items():
        sel = cat == k
        out[..., 0] = np.where(sel, rr, out[..., 0])
        out[..., 1] = np.where(sel, gg, out[..., 1])
        out[..., 2] = np.where(sel, bb, out[..., 2])
    return (out + m[..., None]).astype(f32)


def adjust_hue(rgb, delta):
    """TF adjust_hue_op.cc (CPU) on [..., 3] float32."""
    rgb = np.asarray(rgb, dtype=f32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    lt = r < g
    cases = [  # (condition, vmax, vmid, vmin, category)
        (lt & (b < r), g, r, b, 1), (lt & ~(b < r) & (b > g), b, g, r, 3), (lt & ~(b < r) & ~(b > g), g, b, r, 2),
        (~lt & (b < g), r, g, b, 0), (~lt & ~(b < g) & (b > r), b, r, g, 4), (~lt & ~(b < g) & ~(b > r), r, b, g, 5)]
    vmax, vmid, vmin = (np.zeros_like(r) for _ in range(3))
    cat = np.zeros(r.shape, np.int32)
    for cond, a, m, n, k in cases:
        vmax, vmid, vmin = np.where(cond, a, vmax), np.where(cond, m, vmid), np.where(cond, n, vmin)
        cat = np.where(cond, k, cat)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = (vmid - vmin) / (vmax - vmin)
    h = cat.astype(f32) + np.where(cat % 2 == 0, ratio, f32(1.0) - ratio)
    h = np.where(vmax == vmin, f32(0), h).astype(f32)
    h = h + f32(delta) * f32(6.0)
    while (h < 0).any():
        h = np.where(h < 0, h + f32(6.0), h)
    while (h >= 6).any():
        h = np.where(h >= 6, h - f32(6.0), h)
    hc = h.astype(np.int32)
    ratio = h - hc.astype(f32)
    ratio = np.where(hc % 2 == 1, f32(1.0) - ratio, ratio)
    mid = vmin + ratio * (vmax - vmin)
    tab = {0: (vmax, mid, vmin), 1: (mid, vmax, vmin), 2: (vmin, vmax, mid), 3: (vmin, mid, vmax), 4: (mid, vmin, vmax)}
    out = np.stack([vmax, vmin, mid], -1).astype(f32)            # default: case 5
    for k, (rr, gg, bb) in tab.items():
        sel = hc == k
        out[..., 0] = np.where(sel, rr, out[..., 0])
        out[..., 1] = np.where(sel, gg, out[..., 1])
        out[..., 2] = np.where(sel, bb, out[..., 2])
    return out


# ---- geometry -------------------------------------------------------------------------------------------------------------
def _axis(n_in, n_out):
    s = f32(n_in) / f32(n_out)
    pos = np.arange(n_out, dtype=np.int64).astype(f32) * s
    fl = np.floor(pos)
    lo = np.minimum(np.maximum(fl.astype(np.int64), 0), n_in - 1)
    hi = np.minimum(np.ceil(pos).astype(np.int64), n_in - 1)
    return lo, hi, (pos - fl).astype(f32)


def resize_bilinear(img, out_h, out_w):
    """TF1 ResizeBilinear CPU kernel, align_corners = half_pixel_centers = False, float32 [h, w, c]."""
    img = np.asarray(img, dtype=f32)
    ylo, yhi, ly = _axis(img.shape[0], out_h)
    xlo, xhi, lx = _axis(img.shape[1], out_w)
    lx = lx[None, :, None]
    ly = ly[:, None, None]
    tl, tr = img[ylo][:, xlo], img[ylo][:, xhi]
    bl, br = img[yhi][:, xlo], img[yhi][:, xhi]
    top = tl + (tr - tl) * lx
    bottom = bl + (br - bl) * lx
    return (top + (bottom - top) * ly).astype(f32)


def blur(img, k):
    """conv2d SAME with a k x k box of weight 1 / (k * k), zero padding; summed row by row, left to right."""
    img = np.asarray(img, dtype=f32)
    H, W, _ = img.shape
    p = (k - 1) // 2
    pad = np.zeros((H + k - 1, W + k - 1, 3), f32)
    pad[p:p + H, p:p + W] = img
    w = f32(1.0) / f32(k * k)
    acc = np.zeros_like(img)
    for dy in range(k):
        for dx in range(k):
            acc = acc + pad[dy:dy + H, dx:dx + W] * w
    return acc


# ---- the whole plan -------------------------------------------------------------------------------------------------------
def augment_one(frame_u8, plan, out_h, out_w, gaussian_fn=gaussian):
    """frame_u8: [Hf, Wf, 3] uint8 (the whole frame: plan['row0'] is not applied here) -> float32 [out_h, out_w, 3]."""
    y0, x0, ch, cw = (int(plan[k]) for k in ('y0', 'x0', 'ch', 'cw'))
    x = frame_u8[y0:y0 + ch, x0:x0 + cw].astype(f32) * K255
    if int(plan['rescale']):
        x = resize_bilinear(x, out_h, out_w)
    else:
        assert x.shape[:2] == (out_h, out_w)
    if int(plan['flip']):
        x = x[:, ::-1]
    k = int(plan['blur_k'])
    if k:
        x = blur(x, k)
    x = np.ascontiguousarray(x, dtype=f32)
    op, cp = int(plan['color_op']), f32(plan['color_param'])
    if op == 1:
        x = adjust_saturation(x, cp)
    elif op == 2:
        x = x + cp
    elif op == 3:
        x = adjust_hue(x, cp)
    op, amount, key = int(plan['noise_op']), f32(plan['noise_param']), int(plan['noise_key'])
    if op == 1:
        e = np.arange(out_h * out_w * 3, dtype=np.uint32).reshape(out_h, out_w, 3)
        x = np.where(uniform(key, e, P_SALT) < amount, f32(1.0), x)
        x = np.where(uniform(key, e, P_PEPPER) < amount, f32(0.0), x)
    elif op == 2:
        p = np.arange(out_h * out_w, dtype=np.uint32).reshape(out_h, out_w)
        salt = np.where(uniform(key, p, P_SALT) < amount, f32(1.0), f32(0.0))
        pepper = np.where(uniform(key, p, P_PEPPER) < amount, f32(-1.0), f32(0.0))
        x = np.maximum(np.minimum(x + (salt + pepper)[..., None], f32(1.0)), f32(0.0))
    elif op == 3:
        e = np.arange(out_h * out_w * 3, dtype=np.uint32).reshape(out_h, out_w, 3)
        x = x + gaussian_fn(key, e) * amount
    return x.astype(f32)


def augment_batch(frames_u8, plans, out_h, out_w):
    return np.stack([augment_one(frames_u8[b], plans[b], out_h, out_w) for b in range(len(plans))])
