"""The live-forecast kernels (csrc/live.hip) called through their thin hip.py wrappers on operands laid out by
tests/helpers/layouts.py (NaN around every float input, the sentinel around every output, 0 around the index tables).
Nothing here uses LiveFramePacker or LiveForecaster: the channel table is restated from include/gcl.h.

Rules:
  live_frame_pack     bit-equal (torch.equal) to the window the reference's own extract_live_channels + normalize_frame
                      produced (tests/golden/live_vectors.npz); everything outside the written columns keeps its bits
  live_region_stats   min / max bit-equal to numpy on the same float32 values; mean within 1e-12 mean(|v|) of numpy's
                      float64 mean of them (a reordered float64 sum), and the reference's own float32 .mean() within
                      n 2^-24 mean(|v|) of it (the bound of a float32 sum of n terms)
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import live_case as LC  # noqa: E402
from layouts import DEV, NAN, SENT, Field4, Guarded, Rows, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
C = len(LC.VAR_ORDER)  # 21


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(scope="module")
def gv():
    return LC.golden()


def operands(cycle, rows=None):
    """The device operands of one cycle, every input inside a NaN-guarded buffer: (arena, statics, chan, div, pos, w,
    mean, std, G).  rows: the nodes to keep (None: all 700)."""
    from graphcast_lite_amd import live

    lat, lon = LC.nodes()
    if rows is not None:
        lat, lon = lat[rows], lon[rows]
    G = lat.size
    fields = LC.analysis(cycle)
    st = LC.statics(700)
    kinds, tabs, parts = {}, [], []
    chan = np.zeros((C, 3), dtype=np.int64)
    div = np.ones(C, dtype=np.float32)
    off = 0
    for c, name in enumerate(LC.VAR_ORDER):
        if name in LC.STATIC:
            chan[c] = (2, LC.STATIC.index(name), 0)
        elif name in fields:
            values, lats, lons = fields[name]
            k = LC.kind_of(name)
            if k not in kinds:
                kinds[k] = len(tabs)
                tabs.append(live.point_tables(lats, lons, lat, lon))
            chan[c] = (1, off, kinds[k])
            parts.append(values.reshape(-1))
            off += values.size
            div[c] = 100.0 if name in ("msl", "sp") else 1.0
    assert len(tabs) == 3  # three source grids
    mean, std = LC.scalers()
    statics = np.stack([st[n] if rows is None else st[n][rows] for n in LC.STATIC])
    g = lambda a, dt, fill: Guarded(a.shape, dt, fill, torch.from_numpy(np.ascontiguousarray(a))).view  # noqa: E731
    return (g(np.concatenate(parts), torch.float32, NAN), g(statics, torch.float32, NAN),
            g(chan, torch.int64, 0), g(div, torch.float32, NAN),
            g(np.stack([t[0] for t in tabs]), torch.int32, 0), g(np.stack([t[1] for t in tabs]), torch.float64, NAN),
            g(mean, torch.float32, NAN), g(std, torch.float32, NAN), G)


@pytest.mark.parametrize("layout", ["contig", "pad_nan", "offset", "odd_ld"])
def test_frame_pack_window_equals_the_reference(hip, gv, layout):
    """nd = 1: two launches fill the two slots of a [700, 2 * 21] window whose rows may be padded or offset."""
    want = torch.from_numpy(gv["input_tensor"]).to(DEV)
    out = Rows(700, LC.OBS * C, layout, SENT, role="out")
    assert (layout == "contig") == (out.ld == LC.OBS * C)
    for k in range(LC.OBS):
        *ops, G = operands(k)
        hip.live_frame_pack(*ops, out.view, [k * C], out.ld, G, C)
    assert torch.equal(out.view, want)
    assert out.untouched(SENT)


def test_frame_pack_two_destinations_in_one_launch(hip, gv):
    """nd = 2: cycle 0 into both slots with one launch; both hold the reference's slot 0, the guard columns stay."""
    want = torch.from_numpy(gv["input_tensor"][:, :C]).to(DEV)
    out = Rows(700, LC.OBS * C, "pad_nan", SENT, role="out")
    *ops, G = operands(0)
    hip.live_frame_pack(*ops, out.view, [0, C], out.ld, G, C)
    assert torch.equal(out.view[:, :C], want) and torch.equal(out.view[:, C:], want)
    assert out.untouched(SENT)


def test_frame_pack_batched_destinations(hip, gv):
    """Destinations in different samples of a [3, 700, 42] batch (what hindcast asks for): only those slots change."""
    want = torch.from_numpy(gv["input_tensor"][:, C:]).to(DEV)
    out = Rows(700, LC.OBS * C, "pad_nan", SENT, role="out", B=3)
    *ops, G = operands(1)
    hip.live_frame_pack(*ops, out.view, [1 * out.bs + C, 2 * out.bs], out.ld, G, C)
    assert torch.equal(out.view[1, :, C:], want) and torch.equal(out.view[2, :, :C], want)
    assert bool((out.view[0] == SENT).all()) and bool((out.view[1, :, :C] == SENT).all())
    assert bool((out.view[2, :, C:] == SENT).all()) and out.untouched(SENT)


@pytest.mark.parametrize("node", [0, 690, 699])
def test_frame_pack_single_node(hip, gv, node):
    """G = 1: one node (a seeded one, the north pole, the last) gives that node's row of the reference."""
    out = Guarded((1, LC.OBS * C))
    for k in range(LC.OBS):
        *ops, G = operands(k, rows=np.array([node]))
        assert G == 1
        hip.live_frame_pack(*ops, out.view, [k * C], LC.OBS * C, G, C)
    assert torch.equal(out.view[0], torch.from_numpy(gv["input_tensor"][node]).to(DEV))
    assert out.untouched()


def test_frame_pack_without_fields(hip):
    """No field channel at all (arena and tables NULL): statics and zero fill, z-scored."""
    mean, std = LC.scalers()
    st = LC.statics(700)
    chan = np.zeros((C, 3), dtype=np.int64)
    chan[7], chan[8] = (2, 0, 0), (2, 1, 0)
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    out = Guarded((700, C))
    hip.live_frame_pack(None, dev(np.stack([st["z_surf"], st["lsm"]])), dev(chan), dev(np.ones(C, np.float32)), None,
                        None, dev(mean), dev(std), out.view, [0], C, 700, C)
    frame = np.zeros((700, C), dtype=np.float32)
    frame[:, 7], frame[:, 8] = st["z_surf"], st["lsm"]
    assert torch.equal(out.view, dev((frame - mean[None, :C]) / std[None, :C])) and out.untouched()


def test_frame_pack_rejects_destinations_outside_the_buffer(hip):
    *ops, G = operands(0)
    out = torch.full((700, LC.OBS * C), SENT, device=DEV)
    with pytest.raises(ValueError, match="leave the output buffer"):
        hip.live_frame_pack(*ops, out, [C + 1], LC.OBS * C, G, C)
    with pytest.raises(ValueError, match="leave the output buffer"):
        hip.live_frame_pack(*ops, out, [-1], LC.OBS * C, G, C)
    with pytest.raises(ValueError, match="destinations"):
        hip.live_frame_pack(*ops, out, [0] * (hip.live_max_dest() + 1), LC.OBS * C, G, C)
    with pytest.raises(ValueError, match="destinations"):
        hip.live_frame_pack(*ops, out, [], LC.OBS * C, G, C)
    assert bool((out == SENT).all())


# ----------------------------------------------------------------------------------------------------------------------
# gcl_live_region_stats
# ----------------------------------------------------------------------------------------------------------------------
B, S, G_ = 3, 4, 700
CHANS = (0, 1, 2, 3)
OFFS = np.array([-273.15, 0.0, 0.0, 0.0], dtype=np.float32)


@pytest.fixture(scope="module")
def stats_pred():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((B, G_, S, C))
    x[..., 0] = 263.0 + 9.0 * x[..., 0]
    x[..., 1:3] *= 5.0
    x[..., 3] = 1012.0 + 11.0 * x[..., 3]
    return x.astype(np.float32)


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_region_stats(hip, stats_pred, n, pad):
    rows = np.sort(np.random.default_rng(n).permutation(G_)[:n]).astype(np.int32)
    P = Field4.of(torch.from_numpy(stats_pred).to(DEV), pad=pad)
    out = Guarded((B, S, len(CHANS), 3), torch.float64, fill=-1.0)
    dev = lambda a, dt: Guarded(a.shape, dt, 0 if dt == torch.int32 else NAN, torch.from_numpy(a)).view  # noqa: E731
    got = hip.live_region_stats(P.view, dev(rows, torch.int32), dev(np.array(CHANS, np.int32), torch.int32),
                                dev(OFFS, torch.float32), out=out.view).cpu().numpy()
    assert out.untouched() and P.untouched()
    again = hip.live_region_stats(P.view, dev(rows, torch.int32), dev(np.array(CHANS, np.int32), torch.int32),
                                  dev(OFFS, torch.float32))
    assert same_bits(again, out.view)  # the same bits on every run
    for k, ch in enumerate(CHANS):
        v = stats_pred[..., ch][:, rows, :]  # [B, n, S]
        if ch == 0:
            v = v - 273.15  # float32, as :552-553
        assert v.dtype == np.float32
        v = np.moveaxis(v, 1, 2)  # [B, S, n]
        scale = np.abs(v).astype(np.float64).mean(axis=2)
        assert np.array_equal(got[:, :, k, 1].astype(np.float32).view(np.uint32), v.min(axis=2).view(np.uint32))
        assert np.array_equal(got[:, :, k, 2].astype(np.float32).view(np.uint32), v.max(axis=2).view(np.uint32))
        assert np.array_equal(got[:, :, k, 1:], got[:, :, k, 1:].astype(np.float32).astype(np.float64))
        err = np.abs(got[:, :, k, 0] - v.astype(np.float64).mean(axis=2))
        print(f"[region_stats n={n} ch={ch}] worst mean error / bound = {(err / (1e-12 * scale)).max():.3e}")
        assert np.all(err <= 1e-12 * scale)
        ref32 = np.stack([[v[b, s].mean() for s in range(S)] for b in range(B)])
        assert ref32.dtype == np.float32
        assert np.all(np.abs(got[:, :, k, 0] - ref32.astype(np.float64)) <= n * 2.0 ** -24 * scale)


def test_region_stats_rejects_an_empty_row_list(hip, stats_pred):
    P = torch.from_numpy(stats_pred).to(DEV)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="empty row list"):
        hip.live_region_stats(P, i32([]), i32(list(CHANS)), torch.from_numpy(OFFS).to(DEV))
    out = torch.empty(B, S, 4, 3, dtype=torch.float64, device=DEV)
    rc = hip.lib().gcl_live_region_stats(P.data_ptr(), P.stride(0), P.stride(1), P.stride(2), i32([0]).data_ptr(), 0,
                                         i32(list(CHANS)).data_ptr(), torch.from_numpy(OFFS).to(DEV).data_ptr(), 4, S,
                                         out.data_ptr(), B, 0)
    assert rc != 0 and b"empty row list" in hip.lib().gcl_last_error()


def test_region_stats_rejects_indices_outside_the_forecast(hip, stats_pred):
    P = torch.from_numpy(stats_pred).to(DEV)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)  # noqa: E731
    offs = torch.zeros(1, device=DEV)
    for rows, chans, what in (([0, G_], [0], "row index"), ([-1], [0], "row index"), ([0], [C], "channel index"),
                              ([0], [-1], "channel index")):
        with pytest.raises(ValueError, match=what):
            hip.live_region_stats(P, i32(rows), i32(chans), offs)


def test_region_stats_propagates_nan(hip, stats_pred):
    x = torch.from_numpy(stats_pred[:1].copy()).to(DEV)
    x[0, 5, 2, 1] = NAN
    rows = torch.arange(0, 300, dtype=torch.int32, device=DEV)
    got = hip.live_region_stats(x, rows, torch.tensor([1], dtype=torch.int32, device=DEV),
                                torch.zeros(1, device=DEV))
    assert bool(got[0, 2, 0].isnan().all()) and not bool(got[0, [0, 1, 3]].isnan().any())
