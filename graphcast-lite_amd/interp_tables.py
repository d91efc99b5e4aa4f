"""Host tables of bilinear interpolation, as scipy's `RegularGridInterpolator(method="linear")` evaluates it, and the
cache every module keeps them in.  One copy of what carries a bit-for-bit promise: the cells (`find_cells`), the four
corner weights and their order (`bilinear_corners`), and of the plumbing around them (`TableCache`, `device_tables`).

What is a caller's own stays with the caller (`verify.regrid_tables*`, `wrf.wrf_point_tables`, `live.point_tables`,
`downscale.coarse_tables` / `prediction_tables`, `multires.interpolation_tables`): which axis comes first, how corners
become positions, what lies outside.  numpy only; torch is imported when tables are first uploaded.
"""
from collections import OrderedDict

import numpy as np

CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))  # (first, second) offsets in scipy's order of the four corners


def find_cells(grid, x):
    """(cell index, normalised distance) of every x on an ascending axis, as scipy's RegularGridInterpolator finds
    them: the cell [grid[i], grid[i+1]) holding x, clipped to [0, n-2] (x below the first node: cell 0, x on or past
    the last node: cell n-2), distance (x - grid[i]) / (grid[i+1] - grid[i]) in float64 (outside [0, 1] when
    extrapolating)."""
    grid = np.asarray(grid, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if grid.ndim != 1 or grid.size < 2 or not np.all(np.diff(grid) > 0):
        raise ValueError("the source axes must be strictly ascending with at least 2 points")
    i = np.clip(np.searchsorted(grid, x, side="right") - 1, 0, grid.size - 2)
    return i.astype(np.int64), (x - grid[i]) / (grid[i + 1] - grid[i])


def bilinear_corners(first_axis, second_axis, q_first, q_second):
    """(i_first int64 [P], i_second int64 [P], w float64 [P, 4]) of the query points (q_first, q_second), point by
    point: the cell of each point on the two axes and the weights of its corners `CORNERS`, each formed in float64 as
    `(1 * w_first) * w_second` - "first" being the first axis of the scipy interpolator the caller mirrors.  The
    queries broadcast against each other and P runs over the broadcast shape in C order, so a grid of targets is
    `q_first[:, None]`, `q_second[None, :]` (numbered first-major)."""
    i1, y1 = find_cells(first_axis, q_first)
    i2, y2 = find_cells(second_axis, q_second)
    one = np.float64(1.0)
    w1 = (one * (1 - y1), one * y1)
    w2 = (1 - y2, y2)
    w = np.stack([w1[a] * w2[b] for a, b in CORNERS], axis=-1)
    shape = w.shape[:-1]
    return np.broadcast_to(i1, shape).reshape(-1), np.broadcast_to(i2, shape).reshape(-1), w.reshape(-1, 4)


_HELD = {}  # id(pos) -> ((pos, w), {device: (pos_d, w_d)}) of every host pair a TableCache holds


class TableCache:
    """The `max_entries` most recently used (pos, w) host pairs of one module, by key.  The arrays are shared and
    read-only; so are their device copies (`device_tables`), which leave with the entry."""

    def __init__(self, max_entries: int = 16):
        self.max_entries = max_entries
        self.entries = OrderedDict()  # least recently used first

    def __len__(self):
        return len(self.entries)

    @staticmethod
    def array_key(a):
        a = np.ascontiguousarray(a)
        return (a.dtype.str, a.shape, a.tobytes())

    def get(self, key, make):
        """The pair under `key`; on a miss `make()` builds it (what it raises passes through, nothing is stored)."""
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            return hit
        val = make()
        for a in val:
            a.setflags(write=False)
        self.entries[key] = val
        _HELD[id(val[0])] = (val, {})
        while len(self.entries) > self.max_entries:
            _, old = self.entries.popitem(last=False)
            _HELD.pop(id(old[0]), None)
        return val


def device_tables(pos, w, device):
    """(pos, w) as tensors on `device`.  A pair that a `TableCache` holds is uploaded once per device and the same
    tensors are handed out from then on - they are shared and must not be written; any other pair is uploaded."""
    import torch

    device = torch.device(device)
    held = _HELD.get(id(pos))
    memo = held[1] if held is not None and held[0][0] is pos and held[0][1] is w else None
    if memo is not None and device in memo:
        return memo[device]
    # (the cached arrays are read-only: upload copies)
    t = (torch.from_numpy(np.array(pos)).to(device), torch.from_numpy(np.array(w)).to(device))
    if memo is not None:
        memo[device] = t
    return t
