"""The hard per-class NMS pipeline (csrc/tail_kernels.hip pc_*) at its select, tile and class-count edges: the case table that
tests/test_nms_edges_cpu.py and tests/test_nms_edges_gpu.py share.

CASES: name -> builder of (rows [B, N, D] float32, C, mode, max_out, iou_thr, obj_idx, cls_start); case(name) builds it once.
Every input is built from bit patterns and index arithmetic, never from rounded random floats.  Expected results come from
oracle/nms_ref alone (through tests/_nms_per_class_ref.py).  What is restated here in numpy is only WHICH PATH a class takes
on the device -- member count, the level at which the radix select ends, its threshold digits, Cn, tie overflow, tile count,
hand-over to the exact walk -- so that the CPU test can prove that a case reaches what its name says (EXPECT)."""
import functools

import numpy as np

import _nms_per_class_ref as pcr
from oracle import nms_ref

F32 = np.float32
OBJ, CLS = 4, 5                       # small rows: box, score, C class columns, one column behind them
NMS_TOPK, NMS_CAP, NMS_MAXK, PC_DIRECT_C = 4096, 8192, 2048, 8       # csrc/tail_kernels.hip
LOWEST = np.finfo(np.float32).min
HALF = 0x3F000000                     # bit pattern of 0.5; 0.5 .. 0.625 share the key bits 31..21

CASES, GROUP, EXPECT = {}, {}, {}
GENERAL_TOO = set()                   # cases that also run under byolo_plan_opts.nms_general = 1


def bits(u):
    return np.ascontiguousarray(np.asarray(u, dtype=np.int64).astype(np.uint32)).view(np.float32)


def perm(n, k=0):
    """A fixed permutation of 0 .. n-1: i -> (i * p + n // 3) % n with p the k-th number from 0.618 n downwards coprime to n."""
    n = int(n)
    if n == 1:
        return np.zeros(1, np.int64)
    p, left = max(1, int(0.618 * n)), k
    while True:
        if np.gcd(p, n) == 1:
            if left == 0:
                break
            left -= 1
        p = p - 1 if p > 1 else n - 1
    return (np.arange(n, dtype=np.int64) * p + n // 3) % n


def distinct_scores(n, lo=0x3C000000, stride=4096, k=0):
    """n distinct positive scores, bit patterns lo + j * stride, dealt over the rows by perm(n, k)."""
    return bits(lo + perm(n, k) * stride)


def spread_boxes(n):
    """n disjoint boxes: box i in the middle half of cell i of a square grid."""
    g = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    r, c = i // g, i % g
    return np.stack([(r + 0.25) / g, (c + 0.25) / g, (r + 0.75) / g, (c + 0.75) / g], 1).astype(F32)


def cluster_boxes(n):
    """Box i in cluster i % 40: 0.1 x 0.1 boxes on an 8 x 5 grid of centres further apart than a box, moved by at most 0.001
    inside a cluster (IoU inside a cluster > 0.9, between clusters 0)."""
    i = np.arange(n)
    k = i % 40
    cy = 0.1 + 0.2 * (k % 5) + ((i * 37) % 21 - 10) * 1e-4
    cx = 0.06 + 0.12 * (k // 5) + ((i * 53) % 21 - 10) * 1e-4
    return np.stack([cy - 0.05, cx - 0.05, cy + 0.05, cx + 0.05], 1).astype(F32)


def make_rows(boxes, scores, labels, C, tail=True):
    """[N, D]: class column labels[i] 0.75 and the others 0.25; label -1: every class column 0.5 (a tie: no class).  The column
    behind the class columns holds 9.0, above every class score: a classifier that read one column too far would show."""
    n = len(scores)
    rows = np.zeros((n, CLS + C + (1 if tail else 0)), F32)
    rows[:, :4] = boxes
    rows[:, OBJ] = scores
    labels = np.asarray(labels)
    cls = np.full((n, C), 0.25, F32)
    cls[labels < 0] = 0.5
    live = np.nonzero(labels >= 0)[0]
    cls[live, labels[live]] = 0.75
    rows[:, CLS:CLS + C] = cls
    if tail:
        rows[:, -1] = 9.0
    return rows


def member_masks(rows, C, cls_start=CLS, obj_idx=OBJ):
    """[C, N] bool: the rows the device counts into class c -- the class rule and a score that is a candidate."""
    return pcr.class_masks(rows, cls_start, C) & (rows[:, obj_idx] > LOWEST)[None]


def boxes_by_order(n, scores, labels, C, group_start):
    """Disjoint boxes, except that the member at position p of its class's visiting order takes the box of the member at
    position group_start(p) <= p: planted duplicates (IoU 1), so that the kept list is decided deep inside the order."""
    spread = spread_boxes(n)
    boxes = spread.copy()
    labels = np.asarray(labels)
    for c in range(C):
        order = nms_ref.sort_order(np.where(labels == c, scores, np.nan))
        p = np.arange(len(order))
        boxes[order] = spread[order[group_start(p)]]
    return boxes


def pairs(p):                  # positions 2k, 2k + 1 share a box: every second position is kept
    return p - p % 2


def triples(p):
    return p - p % 3


def light(p):                  # position 4k + 3 repeats 4k + 2
    return np.where(p % 4 == 3, p - 1, p)


def triple_then_pairs(p):      # 0 1 2 | 3 4 | 5 6 | ...: the 2048th kept box sits at position 4095
    return np.where(p < 3, 0, 3 + ((p - 3) // 2) * 2)


# ---- which path a class takes (restatement of score_key, pc_offsets, pc_select; never a source of expected results) ----
def score_keys(scores):
    """uint32, ascending == the visiting order (descending score; either zero is +0.0); 0xFFFFFFFF: no candidate."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    u = s.view(np.uint32).copy()
    u[s == 0] = 0
    key = np.where(u >> 31 != 0, u, ~(u | np.uint32(0x80000000))).astype(np.uint32)
    key[~(s > LOWEST)] = 0xFFFFFFFF
    return key


def bit_pattern_keys(scores):
    """The key that orders zeros by their bit pattern (+0.0 in front of -0.0): the nearest wrong neighbour of score_keys."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    u = s.view(np.uint32)
    key = np.where(u >> 31 != 0, u, ~(u | np.uint32(0x80000000))).astype(np.uint32)
    key[~(s > LOWEST)] = 0xFFFFFFFF
    return key


def key_order(keys):
    idx = np.nonzero(keys != 0xFFFFFFFF)[0]
    return idx[np.argsort((keys[idx].astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64), kind="stable")]


def select_path(keys):
    """keys: the score keys of one class's members -> dict(members, level, digits, Cn, overflow, n_cand, more, tiles).
    level None: the whole segment fits the select's LDS (members <= NMS_CAP)."""
    n = len(keys)
    T = (min(n, NMS_TOPK) + 63) // 64
    out = dict(members=n, level=None, digits=[], Cn=n, overflow=False, tiles=T * (T + 1) // 2)
    if n > NMS_CAP:
        keys = keys.astype(np.int64)
        prefix = pmask = below = 0
        for level, (shift, width) in enumerate(((21, 11), (10, 11), (0, 10))):
            nd = 1 << width
            sel = keys[(keys & pmask) == prefix]
            hist = np.bincount((sel >> shift) & (nd - 1), minlength=2048)
            part = hist.reshape(32, 64).sum(1)
            cum, q = below, 0
            while q < 31 and cum + part[q] < NMS_TOPK:
                cum += part[q]; q += 1
            d = q * 64
            while d < q * 64 + 63 and cum + hist[d] < NMS_TOPK:
                cum += hist[d]; d += 1
            prefix |= d << shift; pmask |= (nd - 1) << shift; below = int(cum)
            out["level"], out["Cn"] = level, int(cum + hist[d])
            out["digits"].append(int(d))
            if out["Cn"] <= NMS_CAP:
                break
            if level == 2:
                out["overflow"] = True
        assert out["overflow"] or (out["Cn"] >= NMS_TOPK and out["Cn"] == int(((keys & pmask) <= prefix).sum()))
    out["n_cand"] = 0 if out["overflow"] else out["Cn"]
    out["more"] = out["overflow"] or n > out["Cn"]
    return out


def paths(rows, C, obj_idx=OBJ, cls_start=CLS):
    """[B][C] select_path of every class of every image."""
    return [[select_path(score_keys(rows[b, m, obj_idx])) for m in member_masks(rows[b], C, cls_start, obj_idx)]
            for b in range(rows.shape[0])]


def hands_over(rows_b, mask, path, max_out, iou_thr, obj_idx=OBJ):
    """Whether the class goes on to the exact walk: ties overflow, or its prefix (the best min(n_cand, NMS_TOPK) members) is used
    up with fewer than max_out kept while members remain behind it."""
    if path["overflow"]:
        return True
    kc = min(path["n_cand"], NMS_TOPK)
    if not (path["more"] or path["n_cand"] > kc):
        return False
    order = nms_ref.sort_order(np.where(mask, rows_b[:, obj_idx], np.nan))
    head = np.zeros(len(rows_b), bool)
    head[order[:kc]] = True
    return len(nms_ref.nms_tf(rows_b[:, :4], rows_b[:, obj_idx], max_out, iou_thr, candidates=head)) < max_out


def matrix_grid(B, N, C):
    """(workgroups per image of pc_matrix, its bound on an image's tiles)."""
    words = NMS_TOPK // 64
    max_tiles = min(C * (words * (words + 1) // 2), (N // 64 + C) * (words + 1) // 2 + 1)
    return min(max_tiles, max(512, min(8192, 32768 // B))), max_tiles


def fill_position(rows_b, mask, keep_c, obj_idx=OBJ):
    """Position in the class's visiting order of its last kept box."""
    order = nms_ref.sort_order(np.where(mask, rows_b[:, obj_idx], np.nan))
    return int(np.nonzero(order == keep_c[-1])[0][0])


# ---- the nearest wrong neighbours of the contract (host only: tests/test_nms_edges_cpu.py, sensitivity) ----
def nms_variant(boxes, scores, max_out, iou_thr=0.5, candidates=None, ties="lower", zeros="equal", ge=False, cut=None):
    """oracle/nms_ref.nms_tf_py with one rule bent: ties='higher' (higher index first among equal scores), zeros='bits' (+0.0 in
    front of -0.0), ge (suppress at IoU >= thr), cut (visit only the first `cut` candidates: a prefix with no hand-over).
    Nothing bent: nms_tf_py itself."""
    boxes = np.asarray(boxes, dtype=np.float32)
    s = np.asarray(scores, dtype=np.float32)
    if zeros == "bits":
        order = key_order(bit_pattern_keys(s))
    else:
        order = nms_ref.sort_order(s)
    if ties == "higher":
        idx = np.nonzero(s > LOWEST)[0][::-1]
        order = idx[np.argsort(-s[idx].astype(np.float64), kind="stable")]
    if candidates is not None:
        order = order[np.asarray(candidates, dtype=bool)[order]]
    if cut is not None:
        order = order[:cut]
    thr = F32(iou_thr)
    sel = []
    for c in order:
        if len(sel) >= max_out:
            break
        ok = True
        for j in reversed(sel):
            v = nms_ref.iou_scalar(boxes[c], boxes[j])
            if (v >= thr) if ge else (v > thr):
                ok = False
                break
        if ok:
            sel.append(int(c))
    return np.asarray(sel, dtype=np.int32)


def nonstrict_masks(rows, cls_start, C):
    """Class by non-strict maximum: the first column that attains the maximum, NaN columns passed over."""
    cls = np.asarray(rows, dtype=np.float32)[:, cls_start:cls_start + C]
    arg = np.argmax(np.where(np.isnan(cls), -np.inf, cls), 1)
    return np.stack([arg == c for c in range(C)])


def per_class_variant(rows, C, max_out, iou_thr, obj_idx, cls_start, masks=None, **bent):
    rows = np.asarray(rows, dtype=np.float32)
    masks = pcr.class_masks(rows, cls_start, C) if masks is None else masks
    return [nms_variant(rows[:, :4], rows[:, obj_idx], max_out, iou_thr, candidates=m, **bent).tolist() for m in masks]


# ---- the case table ----
def _case(name, group, general=False, **expect):
    def deco(fn):
        CASES[name] = fn
        GROUP[name] = group
        EXPECT[name] = expect
        if general:
            GENERAL_TOO.add(name)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def case(name):
    rows, C, mode, max_out, thr, obj, cls = CASES[name]()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    rows.setflags(write=False)
    assert rows.ndim == 3 and 1 <= max_out <= NMS_MAXK and (C == 1 or cls + C <= rows.shape[2])
    return rows, C, mode, max_out, thr, obj, cls


def _std(rows, C, max_out, thr=0.5):
    return np.asarray(rows, F32), C, 2, max_out, thr, OBJ, CLS


# zeros -------------------------------------------------------------------------------------------------------------------
NZ, PZ = F32(-0.0), F32(0.0)
DEN = bits([1])[0]                                            # the smallest denormal
BOX_A, BOX_B = (0.1, 0.1, 0.4, 0.4), (0.6, 0.6, 0.9, 0.9)


@_case("zeros_c1_overlap", "zeros", general=True, kept={(0, 0): [0, 4], (1, 0): [0, 1, 4, 5, 2, 6]})
def _zeros_c1_overlap():
    b0 = np.array([BOX_A] * 4 + [BOX_B] * 4, F32)
    s0 = np.array([NZ, PZ, PZ, NZ, NZ, PZ, -1.0, PZ], F32)
    b1 = spread_boxes(8)
    b1[[2, 3]] = BOX_A; b1[[6, 7]] = BOX_B
    b1[[0, 1, 4, 5]] = [(0.45, 0.0, 0.5, 0.05), (0.45, 0.1, 0.5, 0.15), (0.45, 0.2, 0.5, 0.25), (0.45, 0.3, 0.5, 0.35)]
    s1 = np.array([1.0, 0.5, NZ, PZ, 0.25, 0.1, NZ, PZ], F32)
    return _std(np.stack([make_rows(b0, s0, [0] * 8, 1), make_rows(b1, s1, [0] * 8, 1)]), 1, 8)


@_case("zeros_c1_disjoint", "zeros", general=True, kept={(0, 0): [6, 0, 1]})
def _zeros_c1_disjoint():
    s = np.array([NZ, PZ, NZ, PZ, PZ, NZ, DEN, -DEN], F32)
    return _std(make_rows(spread_boxes(8), s, [0] * 8, 1)[None], 1, 3)


@_case("zeros_c1_specials", "zeros", general=True, kept={(0, 0): [0, 4, 7, 6, 5, 2]})
def _zeros_c1_specials():
    s = np.array([np.inf, LOWEST, np.nextafter(F32(LOWEST), F32(0)), np.nan, NZ, -1.5, -DEN, PZ], F32)
    return _std(make_rows(spread_boxes(8), s, [0] * 8, 1)[None], 1, 8)


def _zeros_c3(boxes, tail):
    s = np.array([np.inf, 1.0, 1.0, NZ, PZ, PZ, NZ, NZ], F32)
    rows = make_rows(boxes, s, [0] * 8, 3, tail=tail)
    rows[:, CLS:CLS + 3] = [(PZ, NZ, -1.0),                  # 0.0 against -0.0: a tie at the maximum, no class
                            (np.nan, 0.5, 0.1), (0.1, 0.5, np.nan),      # a NaN in the first / in the last class column
                            (-1.0, PZ, -0.5), (-1.0, PZ, -0.5), (-1.0, PZ, -0.5), (-1.0, PZ, -0.5),      # class 1, maximum 0.0
                            (-1.0, NZ, DEN)]                 # class 2: a denormal above -0.0
    return rows[None]


@_case("zeros_c3_overlap", "zeros", general=True, members=[[0, 4, 1]], kept={(0, 1): [3], (0, 2): [7]})
def _zeros_c3_overlap():
    b = spread_boxes(8)
    b[3:7] = BOX_A
    return _std(_zeros_c3(b, True), 3, 4)


@_case("zeros_c3_disjoint", "zeros", general=True, members=[[0, 4, 1]], kept={(0, 1): [3, 4], (0, 2): [7]}, no_tail=True)
def _zeros_c3_disjoint():                                    # cls_start + C == D: the class columns end the row
    return _std(_zeros_c3(spread_boxes(8), False), 3, 2)


# class counts -------------------------------------------------------------------------------------------------------------
CLASS_COUNTS, CLASS_NS = (8, 9, 10, 127, 128), (1, 63, 64, 65, 255, 256, 257)


def _classes(C, N):
    empty = (0, C // 2, C - 1)                                # no member at the front, in the middle, at the end
    live = np.array([c for c in range(C) if c not in empty])
    i = np.arange(N)
    lab = np.full(N, -1, np.int64)                            # every seventh row belongs to no class
    who = np.nonzero(i % 7 != 3)[0]
    lab[who] = live[(np.arange(len(who)) + 3) % len(live)]
    rows = make_rows(spread_boxes(N), distinct_scores(N), lab, C)
    cls = (((i[:, None] * 31 + np.arange(C)[None] * 17) % 64) / 128.0).astype(F32)       # all below 0.5, ties among them
    m = np.nonzero(lab >= 0)[0]
    cls[m, lab[m]] = 0.75
    cls[lab < 0, 0] = 0.75; cls[lab < 0, C - 1] = 0.75      # the maximum twice, in the first and the last class column
    rows[:, CLS:CLS + C] = cls
    dup = np.nonzero(i % 5 == 4)[0]
    rows[dup, :4] = rows[dup - 1, :4]
    return _std(np.stack([rows, rows[perm(N, 1)]]), C, 4)


for _C in CLASS_COUNTS:
    for _N in CLASS_NS:
        _case("classes_c%d_n%d" % (_C, _N), "classes", empty=(0, _C // 2, _C - 1),
              classifier="direct" if _C <= PC_DIRECT_C else "tiled")(functools.partial(_classes, _C, _N))


# lengths ------------------------------------------------------------------------------------------------------------------
def _lengths(counts, dense):
    N = max(counts) + 7
    imgs = []
    for b, n0 in enumerate(counts):
        lab = np.ones(N, np.int64)
        who = perm(N, 2 + b)
        lab[who[:n0]] = 0
        lab[who[n0]] = -1
        s = distinct_scores(N, k=b)
        imgs.append(make_rows(boxes_by_order(N, s, lab, 2, triples if dense else light), s, lab, 2))
    return _std(np.stack(imgs), 2, 2048 if dense else 1000)


def _tiles(n):
    t = (min(n, NMS_TOPK) + 63) // 64
    return t * (t + 1) // 2


for _cnt in ((63, 64, 65), (4095, 4096, 4097), (8191, 8192, 8193)):
    for _dense in (False, True):
        _case("lengths_%d%s" % (_cnt[1], "_dense" if _dense else ""), "lengths", general=True,
              members=[[n, max(_cnt) + 7 - n - 1] for n in _cnt], distinct=True,
              path={(b, 0): dict(tiles=_tiles(n), overflow=False, **(dict(level=0) if n > NMS_CAP else dict(level=None, Cn=n)))
                    for b, n in enumerate(_cnt)},
              handover={(b, 0): _dense and n > NMS_TOPK for b, n in enumerate(_cnt)})(functools.partial(_lengths, _cnt, _dense))


# select levels ------------------------------------------------------------------------------------------------------------
def _select(u):
    """C = 1; the scores `u` (bit patterns) dealt over the rows; pairs of the visiting order share a box and max_out is 2048,
    so the kept list is decided at positions 0 .. 4094 of the order: by every key the select lets through."""
    N = len(u)
    s = bits(np.asarray(u, np.int64)[perm(N)])
    lab = np.zeros(N, np.int64)
    return _std(make_rows(boxes_by_order(N, s, lab, 1, pairs), s, lab, 1)[None], 1, 2048)


def _digit_scores(spec):
    """spec: (level-1 key digit d, distinct scores, copies of each) -> bit patterns inside [0.5, 0.625)."""
    out = []
    for d, count, copies in spec:
        assert 0 <= d < 2048 and count <= 1024
        out.append(np.repeat(HALF | ((2047 - d) << 10) | (1023 - np.arange(count)), copies))
    return np.concatenate(out)


_case("select_level1", "select", path={(0, 0): dict(members=9000, level=1, Cn=4096, overflow=False)}, fill={(0, 0): 4094})(
    lambda: _select(HALF + np.arange(9000) * 128))
_case("select_level2", "select", path={(0, 0): dict(members=9300, level=2, overflow=False)}, fill={(0, 0): 4094})(
    lambda: _select(HALF + np.arange(9300) % 1024))
_case("select_slot63", "select", path={(0, 0): dict(level=1, digits=[519, 127], Cn=4164, overflow=False)}, fill={(0, 0): 4094})(
    lambda: _select(_digit_scores([(d, 32, 1) for d in range(127)] + [(127, 100, 1)] + [(d, 10, 1) for d in range(128, 628)])))
_case("select_group31", "select", path={(0, 0): dict(level=1, digits=[519, 2000], Cn=4200, overflow=False)}, fill={(0, 0): 4094})(
    lambda: _select(_digit_scores([(d, 2, 1) for d in range(2000)] + [(2000, 200, 1)] + [(d, 85, 1) for d in range(2001, 2048)])))
_case("select_digit2047", "select", path={(0, 0): dict(level=2, digits=[519, 2047, 0], Cn=4099, overflow=False)}, fill={(0, 0): 4094})(
    lambda: _select(_digit_scores([(d, 2, 1) for d in range(2047)] + [(2047, 1024, 5)])))
_case("select_cn_8192", "select", path={(0, 0): dict(level=1, digits=[519, 1000], Cn=8192, overflow=False)}, fill={(0, 0): 4094})(
    lambda: _select(_digit_scores([(d, 4, 1) for d in range(1000)] + [(1000, 1, 4192)] + [(d, 1, 1) for d in range(1001, 1501)])))
_case("select_cn_8193", "select", path={(0, 0): dict(level=2, overflow=True, n_cand=0)}, fill={(0, 0): 4094}, handover={(0, 0): True})(
    lambda: _select(_digit_scores([(d, 4, 1) for d in range(1000)] + [(1000, 1, 4193)] + [(d, 1, 1) for d in range(1001, 1501)])))
_case("select_straddle", "select", path={(0, 0): dict(level=1, digits=[519, 1000], Cn=5000, overflow=False)}, fill={(0, 0): 4094})(
    lambda: _select(_digit_scores([(d, 4, 1) for d in range(1000)] + [(1000, 1, 1000)] + [(d, 4, 1) for d in range(1001, 2001)])))


# the second trip of pc_matrix -----------------------------------------------------------------------------------------------
@_case("matrix_b16", "matrix", grid=(2080, 2048), fill={(b, 0): 4094 for b in range(16)})
def _matrix_b16():
    N = 4100
    s = distinct_scores(N)
    lab = np.zeros(N, np.int64)
    img = make_rows(boxes_by_order(N, s, lab, 1, pairs), s, lab, 1)
    return _std(np.stack([img] + [img[perm(N, b)] for b in range(1, 16)]), 1, 2048)


@_case("matrix_c4", "matrix", grid=(8320, 8192), fill={(0, c): 4094 for c in range(4)})
def _matrix_c4():
    N = 16600
    i = np.arange(N)
    lab = i % 4
    lab[i % 101 == 0] = -1
    s = distinct_scores(N, stride=2048)
    return _std(make_rows(boxes_by_order(N, s, lab, 4, pairs), s, lab, 4)[None], 4, 2048)


# scan_prefix and greedy_walk ------------------------------------------------------------------------------------------------
def _scan(max_out, ndup):
    N = 200
    s = distinct_scores(N)
    lab = np.zeros(N, np.int64)

    def dup(p):                                              # position 10 repeats position 3, position 20 position 5
        g = p.copy()
        if ndup > 0: g[10] = 3
        if ndup > 1: g[20] = 5
        return g
    return _std(make_rows(boxes_by_order(N, s, lab, 1, dup), s, lab, 1)[None], 1, max_out)


for _m, _d in ((64, 0), (64, 1), (64, 2), (65, 0), (65, 1), (1, 0)):
    _case("scan_m%d_at%d" % (_m, _m - 1 + _d), "scan", general=True, fill={(0, 0): _m - 1 + _d})(functools.partial(_scan, _m, _d))


@_case("scan_m2048_exact", "scan", general=True, members=[[2048]], fill={(0, 0): 2047}, handover={(0, 0): False})
def _scan_m2048_exact():                                     # exactly max_out disjoint members: the prefix is used up, nothing behind it
    N = 2060
    s = distinct_scores(N)
    s[perm(N, 3)[:12]] = [np.nan, -np.inf, LOWEST] * 4
    return _std(make_rows(spread_boxes(N), s, [0] * N, 1)[None], 1, 2048)


@_case("scan_m2048_used_up", "scan", general=True, path={(0, 0): dict(members=5000, level=None, n_cand=5000)}, fill={(0, 0): 4095},
       handover={(0, 0): False})
def _scan_m2048_used_up():                                   # the 2048th box is kept at the last position of the prefix, members behind it
    N = 5000
    s = distinct_scores(N)
    lab = np.zeros(N, np.int64)
    return _std(make_rows(boxes_by_order(N, s, lab, 1, triple_then_pairs), s, lab, 1)[None], 1, 2048)


def _clusters(n_members, N, C):
    lab = np.ones(N, np.int64) if C == 2 else np.full(N, 0, np.int64)
    who = perm(N, 1)
    lab[who[:n_members]] = 0
    s = distinct_scores(N)
    boxes = cluster_boxes(N)
    if C == 2:
        lab[who[n_members]] = -1
        last = nms_ref.sort_order(np.where(lab == 0, s, np.nan))[-1]
        boxes[last] = (0.95, 0.95, 0.99, 0.99)               # the last member visited stands alone: kept only if the walk gets there
    else:
        s[who[n_members:]] = np.nan
    return _std(make_rows(boxes, s, lab, C)[None], C, 1000)


_case("walk_clusters_1024", "walk", general=True, members=[[1024]], nkept={(0, 0): 40})(functools.partial(_clusters, 1024, 1030, 1))
_case("walk_clusters_1025", "walk", general=True, members=[[1025]], nkept={(0, 0): 40})(functools.partial(_clusters, 1025, 1030, 1))
_case("walk_clusters_4097", "walk", general=True, members=[[4097, 32]], nkept={(0, 0): 41}, fill={(0, 0): 4096},
      handover={(0, 0): True})(functools.partial(_clusters, 4097, 4130, 2))


# thresholds -----------------------------------------------------------------------------------------------------------------
def _iou_pair(thr):
    """Boxes A = (0, 0, 1, w) and B = (0, 0, 1, x) inside it whose float32 IoU is exactly float32(thr), and a B' whose IoU is
    the next float32 above it.  Found by search over bit patterns, checked with the oracle's IoU."""
    t = F32(thr)
    up = np.nextafter(t, F32(1))
    for m in range(0, 64):
        w = bits([0x3F800000 + m])[0]
        a = np.array([0, 0, 1, w], F32)
        x0 = int(np.array([t * w], F32).view(np.uint32)[0])
        found = {}
        for k in range(-64, 65):
            b = np.array([0, 0, 1, bits([x0 + k])[0]], F32)
            v = nms_ref.iou_scalar(a, b)
            if v == t: found.setdefault("eq", b)
            if v == up: found.setdefault("up", b)
        if len(found) == 2:
            return a, found["eq"], found["up"]
    raise AssertionError("no box pair at IoU == float32(%r) and one ulp above" % thr)


def _threshold(thr):
    a, b_eq, b_up = _iou_pair(thr)
    imgs = []
    for b in (b_eq, b_up):                                   # the pair, and its mirror image (corners flipped) visited B first
        boxes = np.stack([a, b, -b, -a])
        imgs.append(make_rows(boxes, np.array([0.9, 0.8, 0.7, 0.6], F32), [0] * 4, 1))
    return _std(np.stack(imgs), 1, 4, thr)


for _t in (0.5, 0.45, 0.3):                                  # exact; float32(0.45) < 0.45; float32(0.3) > 0.3: both rounding directions
    _case("threshold_%g" % _t, "thresholds", general=True, kept={(0, 0): [0, 1, 2, 3], (1, 0): [0, 2]})(functools.partial(_threshold, _t))


# every regime side by side in one batch ---------------------------------------------------------------------------------------
@_case("batch_regimes", "batch", general=True, members=[[0, 0], [8193, 6], [64, 5]],
       path={(1, 0): dict(level=0, overflow=False), (2, 0): dict(level=None, tiles=1)})
def _batch_regimes():
    N = 8200
    imgs = []
    for b, n0 in enumerate((0, 8193, 64)):
        lab = np.ones(N, np.int64)
        who = perm(N, 2 + b)
        lab[who[:n0]] = 0
        lab[who[8193]] = -1
        s = distinct_scores(N, k=b)
        if b == 0:
            s[:] = np.nan                                    # no candidate at all
        if b == 2:
            s[who[64:8193]] = -np.inf; s[who[8199:]] = np.nan            # 64 members of class 0, 5 of class 1
        imgs.append(make_rows(boxes_by_order(N, s, lab, 2, light), s, lab, 2))
    return _std(np.stack(imgs), 2, 1000)
