"""The case table of tests/_nms_edges.py without a GPU: every case reaches the path its name says (the numpy restatement of the
device's path choice, and the reference's kept list), the two oracles agree on the small cases, every group tells the contract
from its nearest wrong neighbour, and the inputs are ones the reference says something about."""
import numpy as np
import pytest

import _nms_edges as ne
import _nms_per_class_ref as pcr
from oracle import nms_ref

ALL = sorted(ne.CASES)


def _ref(name):
    """[B] of (kept indices, kept per class) from the reference."""
    rows, C, mode, max_out, thr, obj, cls = ne.case(name)
    return [pcr.nms_per_class(rows[b], obj, cls, C, max_out, thr)[1:] for b in range(rows.shape[0])]


def _keep_of(keep, cnt, c):
    lo = int(cnt[:c].sum())
    return keep[lo:lo + int(cnt[c])]


@pytest.mark.parametrize("name", ALL)
def test_case_reaches_what_its_name_says(name):
    rows, C, mode, max_out, thr, obj, cls = ne.case(name)
    exp = ne.EXPECT[name]
    B, N, D = rows.shape
    assert mode == 2 and D == cls + C + (0 if exp.get("no_tail") else 1)
    path = ne.paths(rows, C, obj, cls)
    ref = _ref(name)
    masks = [ne.member_masks(rows[b], C, cls, obj) for b in range(B)]
    print(name, "paths:", [[{k: v for k, v in p.items()} for p in img[:4]] for img in path[:3]])
    # the key restatement orders every image as the reference does
    for b in range(B):
        assert np.array_equal(ne.key_order(ne.score_keys(rows[b, :, obj])), nms_ref.sort_order(rows[b, :, obj]))
    if "members" in exp:
        assert [[p["members"] for p in img] for img in path] == exp["members"]
    if exp.get("distinct"):
        for b in range(B):
            s = rows[b, :, obj]
            assert len(np.unique(s.view(np.uint32))) == N and not (s == 0).any()
    for (b, c), want in exp.get("path", {}).items():
        got = {k: path[b][c][k] for k in want}
        assert got == want, (b, c, path[b][c])
    for (b, c), want in exp.get("handover", {}).items():
        assert ne.hands_over(rows[b], masks[b][c], path[b][c], max_out, thr, obj) == want, (b, c)
    for (b, c), want in exp.get("fill", {}).items():         # the prefix position that fills max_out, off the reference's kept list
        keep_c = _keep_of(*ref[b], c)
        assert len(keep_c) == (max_out if "nkept" not in exp else exp["nkept"][(b, c)])
        assert ne.fill_position(rows[b], masks[b][c], keep_c, obj) == want, (b, c)
    for (b, c), want in exp.get("kept", {}).items():
        assert _keep_of(*ref[b], c).tolist() == want, (b, c)
    for (b, c), want in exp.get("nkept", {}).items():
        assert int(ref[b][1][c]) == want, (b, c)
    if "grid" in exp:                                        # more tiles in an image than pc_matrix has workgroups for it
        tiles, grid = exp["grid"]
        assert ne.matrix_grid(B, N, C)[0] == grid and tiles > grid
        for img in path:
            assert sum(p["tiles"] for p in img) == tiles and tiles <= ne.matrix_grid(B, N, C)[1]
            assert all(not p["overflow"] and p["n_cand"] >= ne.NMS_TOPK for p in img)
    if "empty" in exp:
        assert (C <= ne.PC_DIRECT_C) == (exp["classifier"] == "direct")
        for img in path:
            assert all(img[c]["members"] == 0 for c in exp["empty"])
            assert N < 8 * C or all(img[c]["members"] > 0 for c in range(C) if c not in exp["empty"])
        assert sorted(map(bytes, rows[0])) == sorted(map(bytes, rows[1])) and (N == 1 or not np.array_equal(rows[0], rows[1]))


def test_named_cases_exist():
    """The table holds what the groups promise."""
    assert len([n for n in ALL if ne.GROUP[n] == "classes"]) == len(ne.CLASS_COUNTS) * len(ne.CLASS_NS) == 35
    assert ne.CLASS_COUNTS == (8, 9, 10, 127, 128) and ne.CLASS_NS == (1, 63, 64, 65, 255, 256, 257)
    for n in ("lengths_64", "lengths_4096", "lengths_8192", "lengths_64_dense", "lengths_4096_dense", "lengths_8192_dense"):
        assert n in ne.GENERAL_TOO
    assert {ne.case(n)[3] for n in ALL if ne.GROUP[n] == "scan"} == {1, 64, 65, 2048}
    levels = {n: ne.paths(*[ne.case(n)[i] for i in (0, 1, 5, 6)])[0][0] for n in ALL if ne.GROUP[n] == "select"}
    assert {p["level"] for p in levels.values()} == {1, 2}
    assert any(p["digits"][1] % 64 == 63 and p["digits"][1] // 64 < 31 for p in levels.values())     # last slot of a group
    assert any(p["digits"][1] // 64 == 31 and p["digits"][1] % 64 != 63 for p in levels.values())    # the last group
    assert any(p["digits"][1] == 2047 for p in levels.values())                                      # both loop bounds at once
    assert any(p["Cn"] == ne.NMS_CAP and not p["overflow"] for p in levels.values()) and any(p["overflow"] for p in levels.values())
    assert any(ne.NMS_TOPK < p["n_cand"] < ne.NMS_CAP for p in levels.values())


@pytest.mark.parametrize("name", [n for n in ALL if ne.case(n)[0].shape[1] <= 300])
def test_oracles_agree(name):
    """oracle/nms_ref.nms_tf (C) == nms_tf_py (numpy scalars) == the variant with nothing bent, class by class."""
    rows, C, mode, max_out, thr, obj, cls = ne.case(name)
    for b in range(rows.shape[0]):
        for m in pcr.class_masks(rows[b], cls, C):
            a = nms_ref.nms_tf(rows[b, :, :4], rows[b, :, obj], max_out, thr, candidates=m)
            p = nms_ref.nms_tf_py(rows[b, :, :4], rows[b, :, obj], max_out, thr, candidates=m)
            v = ne.nms_variant(rows[b, :, :4], rows[b, :, obj], max_out, thr, candidates=m)
            assert np.array_equal(a, p) and np.array_equal(a, v)


def _differs(name, masks_fn=None, d_max_out=0, **bent):
    rows, C, mode, max_out, thr, obj, cls = ne.case(name)
    out = False
    for b in range(rows.shape[0]):
        keep, cnt = pcr.nms_per_class(rows[b], obj, cls, C, max_out, thr)[1:]
        want = [_keep_of(keep, cnt, c).tolist() for c in range(C)]
        masks = masks_fn(rows[b], cls, C) if masks_fn else None
        got = ne.per_class_variant(rows[b], C, max_out + d_max_out, thr, obj, cls, masks=masks, **bent)
        out |= got != want
    return out


SENSITIVITY = [          # (group, the bent rule, the cases of the group tried in turn)
    ("zeros", dict(zeros="bits"), ["zeros_c1_overlap", "zeros_c1_disjoint", "zeros_c1_specials", "zeros_c3_overlap", "zeros_c3_disjoint"]),
    ("zeros", dict(ties="higher"), ["zeros_c1_overlap", "zeros_c3_disjoint"]),
    ("zeros", dict(masks_fn=ne.nonstrict_masks), ["zeros_c3_overlap", "zeros_c3_disjoint"]),
    ("classes", dict(masks_fn=ne.nonstrict_masks), ["classes_c8_n65", "classes_c9_n65", "classes_c128_n257"]),
    ("classes", dict(d_max_out=1), ["classes_c9_n257"]),
    ("classes", dict(d_max_out=-1), ["classes_c9_n257"]),
    ("select", dict(ties="higher"), ["select_straddle"]),
    ("scan", dict(d_max_out=1), ["scan_m64_at63", "scan_m65_at65", "scan_m1_at0"]),
    ("scan", dict(d_max_out=-1), ["scan_m64_at64", "scan_m65_at64"]),
    ("thresholds", dict(ge=True), ["threshold_0.5", "threshold_0.45", "threshold_0.3"]),
    ("walk", dict(cut=ne.NMS_TOPK), ["walk_clusters_4097"]),
]


@pytest.mark.parametrize("group,bent,names", SENSITIVITY, ids=["%s-%s" % (g, "-".join(sorted(b))) for g, b, _ in SENSITIVITY])
def test_group_tells_the_contract_from_its_neighbour(group, bent, names):
    """The reference with one rule bent keeps another list on at least one case of the group the rule belongs to."""
    assert all(ne.GROUP[n] == group for n in names)
    hit = [n for n in names if _differs(n, **bent)]
    print("%s: %s changes the kept list of %s" % (group, bent, hit))
    assert hit
    if bent == dict(zeros="bits"):                           # what a device that orders zeros by bit pattern gets wrong: all five
        assert hit == names
    if "ge" in bent or "d_max_out" in bent:
        assert hit == names


def test_zeros_by_bit_pattern_touch_only_the_zeros_cases():
    """Ordering zeros by bit pattern changes the visiting order of the zeros cases and of no other case: no other case holds a
    zero score among its candidates."""
    for name in ALL:
        rows, C, mode, max_out, thr, obj, cls = ne.case(name)
        same = all(np.array_equal(ne.key_order(ne.bit_pattern_keys(rows[b, :, obj])), ne.key_order(ne.score_keys(rows[b, :, obj])))
                   for b in range(rows.shape[0]))
        assert same == (ne.GROUP[name] != "zeros"), name


@pytest.mark.parametrize("name", ALL)
def test_inputs_fit_the_reference(name):
    rows, C, mode, max_out, thr, obj, cls = ne.case(name)
    assert any(p["members"] > 0 for img in ne.paths(rows, C, obj, cls) for p in img)
    if C > 1:
        for b in range(rows.shape[0]):
            assert pcr.dropped_share(rows[b], cls, C) < 0.5
    assert (rows[..., :4] == rows[..., :4]).all()            # boxes are plain numbers; only scores and class scores hold NaN
