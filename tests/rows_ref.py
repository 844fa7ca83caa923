"""The contract "Rows back to texts" (include/bpe_gpu.h) in plain Python: a loop over the rows and their cells.  The
yardstick of tests/test_rows_host.py and tests/test_gpu_rows.py; it shares no code with the library."""
import numpy as np


class RowsError(Exception):
    """code: "EINVAL" (a window above L) or "EDATA" (a kept cell that is no id); row: the lowest offending row"""

    def __init__(self, code, row):
        super().__init__(f"{code} at row {row}")
        self.code, self.row = code, row


def unpack(rows, lens=None, pad_id=None, stop_ids=(), skip_ids=None):
    """(ids uint32[n], text_off uint64[B + 1], bounds uint32[B, 2]) of a 2-D integer array; a cell is an id when its
    value (as the signed 64-bit number a 64-bit cell holds, or the unsigned 32-bit number a 32-bit cell holds) lies in
    0 .. 2^32 - 1"""
    rows = np.asarray(rows)
    B, L = rows.shape
    if rows.dtype == np.uint64:
        rows = rows.view(np.int64)
    elif rows.dtype == np.int32:
        rows = rows.view(np.uint32)
    if lens is not None:
        for k in range(B):
            if int(lens[k]) > L:
                raise RowsError("EINVAL", k)
    stops = {int(s) for s in stop_ids}
    if pad_id is not None:
        stops.add(int(pad_id))
    skips = set() if skip_ids is None else {int(s) for s in skip_ids}
    ids, text_off, bounds = [], [0], []
    for k in range(B):
        cells = [int(x) for x in rows[k, :L if lens is None else int(lens[k])]]
        a = 0
        if pad_id is not None:
            while a < len(cells) and cells[a] == int(pad_id):
                a += 1
        z = a
        while z < len(cells) and cells[z] not in stops:
            z += 1
        for x in cells[a:z]:
            if x in skips:
                continue
            if not 0 <= x <= 0xFFFFFFFF:
                raise RowsError("EDATA", k)
            ids.append(x)
        text_off.append(len(ids))
        bounds.append((a, z))
    return (np.array(ids, dtype=np.uint32), np.array(text_off, dtype=np.uint64),
            np.array(bounds, dtype=np.uint32).reshape(B, 2))


def batch(rng, B, L, dtype, pad_id, stop_ids, skip_ids, vocab=300, garbage=True):
    """rows[B, L] of `dtype` that hold every kind of row the contract speaks of, in turn: all pad, no stop, a stop at
    column 0, a stop at L - 1, a pad in the role of the stop (left padding, text, pad), and random ones (left padding of
    a random length, a text with skipped ids in it, a stop, then garbage: for 64-bit cells values that are no id)"""
    pad = 0 if pad_id is None else int(pad_id)
    plain = [x for x in range(vocab) if x != pad and x not in set(stop_ids) and x not in set(skip_ids or ())]
    body = np.array(plain + list(skip_ids or ())[:4] * 8, dtype=np.int64)
    rows = np.zeros((B, L), dtype=np.int64)
    for k in range(B):
        row = rng.choice(body, L)
        kind = k % 7
        if kind == 0:
            row[:] = pad
        elif kind == 1:
            pass
        elif kind == 2 and L and len(stop_ids):
            row[0] = stop_ids[0]
        elif kind == 3 and L and len(stop_ids):
            row[L - 1] = stop_ids[-1]
        elif kind == 4 and L:
            lead, end = int(rng.integers(0, L + 1)), int(rng.integers(0, L + 1))
            row[:lead] = pad
            row[max(lead, end):] = pad
        elif L:
            lead, end = int(rng.integers(0, L + 1)), int(rng.integers(0, L + 1))
            row[:lead] = pad
            if end >= lead and end < L:
                row[end] = stop_ids[int(rng.integers(0, len(stop_ids)))] if len(stop_ids) else pad
                # (a pad right behind the leading pads would only lengthen them: the cells behind it are text then)
                lengthens = pad_id is not None and row[end] == pad and end == lead
                if garbage and np.dtype(dtype).itemsize == 8 and (len(stop_ids) or pad_id is not None) and not lengthens:
                    row[end + 1:] = rng.choice(np.array([-100, 1 << 40, -1, 1 << 32, 7], dtype=np.int64), L - end - 1)
        rows[k] = row
    if np.dtype(dtype) == np.uint64:
        return rows.view(np.uint64).copy()
    return rows.astype(dtype)
