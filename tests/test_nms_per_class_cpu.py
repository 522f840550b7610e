"""BYOLO_NMS_PER_CLASS without a GPU: the declarations (header, ctypes table, exported symbols), the per-class reference of
the GPU tests against the two pinned modes of oracle/nms_ref and on hand cases of the class rule, the capacity arithmetic
of an engine in this mode and the world-2 gloo gather of box lists of that capacity."""
import os
import re
import socket
import subprocess
import sys

import numpy as np

import _nms_per_class_ref as pcr
from _nms_per_class_ref import OBJ_IDX, CLS_START
from conftest import REPO

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRY_POINTS = ("byolo_nms_workspace_bytes_ex", "byolo_nms_class_counts")


def test_header_prototypes_and_exports_agree():
    from byolo import _lib
    import byolo
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "byolo.h")).read(), flags=re.S)
    enum = re.search(r"enum\s*\{([^}]*BYOLO_NMS_AGNOSTIC[^}]*)\}", text).group(1)
    modes = {k.strip(): int(v) for k, v in (e.split("=") for e in enum.split(","))}
    assert modes == {"BYOLO_NMS_AGNOSTIC": 0, "BYOLO_NMS_TWO_CLASS": 1, "BYOLO_NMS_PER_CLASS": 2}
    assert (_lib.NMS_AGNOSTIC, _lib.NMS_TWO_CLASS, _lib.NMS_PER_CLASS) == (0, 1, 2) and byolo.NMS_PER_CLASS == 2
    limit = int(re.search(r"#define\s+BYOLO_NMS_MAX_CLASSES\s+(\d+)", text).group(1))
    assert limit == _lib.NMS_MAX_CLASSES and limit >= 128            # the largest class count the decode tests use
    assert re.search(r"#define\s+BYOLO_ABI_VERSION\s+7\b", text) and _lib.lib.byolo_abi_version() == 7       # additive
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_ENTRY_POINTS:
        m = re.search(r"BYOLO_API\s+[\w\s\*]+?\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.PROTOTYPES[name][1]), name
        assert name in exported and hasattr(_lib.lib, name)


def test_workspace_sizes():
    """The old entry point returns what it returned; its sibling agrees with it in the two old modes, sizes the per-class mode
    by the class count, and has no size for a class count the mode refuses."""
    from byolo import _lib
    ex, old = _lib.lib.byolo_nms_workspace_bytes_ex, _lib.lib.byolo_nms_workspace_bytes
    for B, N in ((1, 1), (2, 22743), (11, 120960)):
        assert ex(B, N, 0, 2) == ex(B, N, 1, 2) == ex(B, N, 0, 80) == old(B, N) > 0
        sizes = [ex(B, N, 2, C) for C in (1, 2, 3, 80, 128)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert ex(2, 22743, 2, 0) == 0 and ex(2, 22743, 2, _lib.NMS_MAX_CLASSES + 1) == 0 and ex(0, 22743, 2, 3) == 0


def test_reference_two_classes_is_the_two_class_oracle():
    from oracle import nms_ref
    rows = pcr.random_rows(np.random.default_rng(1), 2, 6000, 2)
    for b in range(2):
        share = pcr.dropped_share(rows[b], CLS_START, 2)
        assert 0.0 < share < 0.5, share
        r_rows, r_keep, n0 = nms_ref.nms_two_class(rows[b], OBJ_IDX, CLS_START, 1000)
        p_rows, p_keep, p_cnt = pcr.nms_per_class(rows[b], OBJ_IDX, CLS_START, 2, 1000)
        assert np.array_equal(p_keep, r_keep) and int(p_cnt[0]) == n0 and int(p_cnt.sum()) == len(r_keep)
        assert np.array_equal(p_rows.view(np.uint32), r_rows.view(np.uint32))
        assert p_cnt[0] == 1000 and len(r_keep) > 1000           # the raised class fills max_out, the other adds to it


def test_reference_one_class_is_the_agnostic_oracle():
    from oracle import nms_ref
    rows = pcr.random_rows(np.random.default_rng(2), 1, 6000, 1)[0]
    rows[::7, CLS_START] = np.nan                              # one class: a NaN class score does not drop the row
    r_rows, r_keep = nms_ref.nms_agnostic(rows, OBJ_IDX, 300)
    p_rows, p_keep, p_cnt = pcr.nms_per_class(rows, OBJ_IDX, CLS_START, 1, 300)
    assert np.array_equal(p_keep, r_keep) and p_cnt.tolist() == [len(r_keep)] == [300]
    assert np.array_equal(p_rows.view(np.uint32), r_rows.view(np.uint32), )
    assert pcr.dropped_share(rows, CLS_START, 1) == 0.0


def test_class_rule_hand_cases():
    """Row i belongs to class c iff cls[i][c] > cls[i][k] for every k != c, strictly, in float32."""
    C = 4
    rows = np.zeros((6, pcr.row_len(C)), np.float32)
    for i in range(6):                                         # six boxes far apart: nothing suppresses anything
        rows[i, 0:4] = (0.1 * i, 0.1 * i, 0.1 * i + 0.05, 0.1 * i + 0.05)
        rows[i, OBJ_IDX] = 0.9 - 0.1 * i
    cls = rows[:, CLS_START:CLS_START + C]
    cls[0] = (0.1, 0.7, 0.2, 0.3)                              # class 1
    cls[1] = (0.7, 0.2, 0.7, 0.1)                              # a two-way tie at the maximum: no class
    cls[2] = (0.9, np.nan, 0.1, 0.2)                           # a NaN class score (not at the maximum): no class
    cls[3] = (0.1, 0.2, 0.3, 0.8)                              # the maximum in the LAST class
    cls[4] = (0.5, 0.5 - 2.0 ** -25, 0.1, 0.2)                 # float32: 0.5 - 2^-25 is its own value below 0.5 -> class 0
    cls[5] = (np.float32(0.3) + np.float32(1e-9), 0.3, 0.1, 0.2)      # float32: the sum rounds back to 0.3 -> tie, no class
    masks = pcr.class_masks(rows, CLS_START, C)
    assert masks.astype(int).tolist() == [[0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0]]
    k_rows, keep, cnt = pcr.nms_per_class(rows, OBJ_IDX, CLS_START, C)
    assert keep.tolist() == [4, 0, 3] and cnt.tolist() == [1, 1, 0, 1]          # class order, not score order
    assert np.array_equal(k_rows, rows[[4, 0, 3]])
    assert abs(pcr.dropped_share(rows, CLS_START, C) - 0.5) < 1e-12


def test_engine_capacity():
    """Rows per image of the NMS outputs: max_out per class."""
    from byolo import Engine, NMS_AGNOSTIC, NMS_TWO_CLASS, NMS_PER_CLASS
    assert Engine((64, 64, 3), 3, nms_mode=NMS_PER_CLASS).out_cap == 3000
    assert Engine((64, 64, 3), 80, nms_mode=NMS_PER_CLASS, max_out=100).out_cap == 8000
    assert Engine((64, 64, 3), 1, nms_mode=NMS_PER_CLASS, max_out=7).out_cap == 7
    assert Engine((64, 64, 3), 2, nms_mode=NMS_TWO_CLASS).out_cap == 2000 and Engine((64, 64, 3), 5, nms_mode=NMS_AGNOSTIC).out_cap == 1000
    assert Engine.nms_cap(NMS_PER_CLASS, 2048, 128) == 2048 * 128 and Engine.nms_cap(NMS_TWO_CLASS, 10, 128) == 20


def test_inference_helper_modes():
    """byolo.inference.nms: per_class=True asks for mode 2, two_class=True keeps meaning mode 1."""
    from byolo import inference as binf

    class _T:
        def __init__(self, shape): self.shape = shape
        def dim(self): return len(self.shape)
        def contiguous(self): return self
        def __getitem__(self, k): return self

    class _Cnt:
        def __getitem__(self, k): return self
        def cpu(self): return self
        def tolist(self): return [0]

    class _Eng:
        def sort_nms(self, b, obj_idx, cls_start_idx, nms_mode, max_out):
            self.mode = nms_mode
            return {"count": _Cnt(), "rows": _T((1, 0, 5))}

    class _M:
        engine, obj_idx, cls_start_idx = _Eng(), 4, 5

    for kw, mode in ((dict(), 0), (dict(two_class=True), 1), (dict(per_class=True), 2)):
        binf.nms(_T((1, 10, 8)), _M, batched=True, **kw)
        assert _M.engine.mode == mode


def test_gather_world2_three_classes(tmp_path):
    import torch
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_nms_per_class_worker.py"), str(r), "2", str(port), str(tmp_path)],
                              env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    for r in range(2):
        res = torch.load(os.path.join(tmp_path, "rank%d.pt" % r))
        assert res["cap"] == 12 and res["g_rows_shape"] == (4, 12, 9) and res["g_kept_shape"] == (4, 12)
        assert [len(k) for k in res["u_kept"]] == [12, 11, 10]                     # image 0: all C * max_out rows arrive
        for g in range(3):
            assert res["u_kept"][g].tolist() == [1000 * g + i for i in range(12 - g)]
            assert torch.equal(res["u_rows"][g], (100.0 * g + torch.arange(9, dtype=torch.float32)).expand(12 - g, 9))
