"""What the two recalibrations share on the Python side (byolo/recalibrate.py: the variances; byolo/score_recal.py: the score): the
JSON file of a calibration, and the launch of a fit that runs one workgroup per segment of records ordered by group."""
import ctypes
import json
import math

import numpy as np

from ._lib import ByoloError, lib


def raise_last(rc):
    """ByoloError with the library's message when a handle-less call returned rc < 0."""
    if rc < 0:
        msg = lib.byolo_last_error(None)
        raise ByoloError(rc, msg.decode('utf-8', 'replace') if msg else '?')


def check_min_n(prefix, min_n):
    if isinstance(min_n, bool) or not isinstance(min_n, (int, np.integer)) or min_n < 1:
        raise ValueError('%s: min_n is an integer >= 1, not %r' % (prefix, min_n))


def _clean(v):
    """A report value as JSON takes it: a non-finite float becomes None, inside a list as well."""
    if isinstance(v, float) and not math.isfinite(v):
        return None
    return [_clean(x) for x in v] if isinstance(v, list) else v


class Calibration:
    """A fitted table with what it was fitted for and the per-group report, kept as JSON.  A subclass names its FORMAT, the PREFIX
    of its messages and the keys a file must have (REQUIRED), lists its fields in file order (`_fields`) and builds itself from a
    file's dict (`_from_dict`)."""

    # ---- JSON: Python writes a float as its repr, which reads back to the same bits -------------------------------------------------
    def to_json(self):
        d = {'format': self.FORMAT, 'version': 1}
        d.update(self._fields())
        d['report'] = [{k: _clean(v) for k, v in e.items()} for e in self.report]
        return json.dumps(d, indent=1, allow_nan=False)

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        if not isinstance(d, dict) or d.get('format') != cls.FORMAT:
            raise ValueError('%s: format: not a %s file' % (cls.PREFIX, cls.FORMAT))
        for k in cls.REQUIRED:
            if k not in d:
                raise ValueError('%s: the file has no %r' % (cls.PREFIX, k))
        return cls._from_dict(d)

    def save(self, path):
        with open(path, 'w') as f:
            f.write(self.to_json() + '\n')

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.from_json(f.read())

    @classmethod
    def coerce(cls, cal):
        """A calibration of this class from one, from a path, or from the dict of to_json()."""
        if isinstance(cal, cls):
            return cal
        if isinstance(cal, dict):
            return cls.from_json(json.dumps(cal))
        if isinstance(cal, (str, bytes)) or hasattr(cal, '__fspath__'):
            return cls.load(cal)
        raise ValueError('%s: a %s, a path or a dict, not %r' % (cls.PREFIX, cls.__name__, type(cal).__name__))


def segmented_fit(columns, group, n_groups, words, workspace_bytes, launch):
    """One launch of a fit kernel that runs a workgroup per group.  columns: device tensors [n] or [n, K], one row per record; group
    [n]: the records' group in [0, n_groups) (any integer dtype).  The records are ordered by group with a stable sort, so every
    group keeps the order it came in.  launch(columns, seg, out, ws, stream) -- device pointers: the ordered columns, the n_groups + 1
    segment offsets, out [n_groups, words] float64, a workspace of workspace_bytes -- makes the library call on the current stream
    and returns its code (ByoloError below 0).  Returns out as a numpy array."""
    import torch
    dev = columns[0].device
    g = group.to(torch.int64)
    order = torch.sort(g, stable=True)[1]
    cols = [c[order].contiguous() for c in columns]
    seg = torch.zeros(n_groups + 1, dtype=torch.int64, device=dev)
    if g.numel():
        seg[1:] = torch.cumsum(torch.bincount(g, minlength=n_groups)[:n_groups], 0)
    out = torch.empty((n_groups, words), dtype=torch.float64, device=dev)
    ws = torch.empty(max(workspace_bytes // 8, 1), dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    raise_last(launch([p(c) for c in cols], p(seg), p(out), p(ws), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out.cpu().numpy()                                       # the host wait
