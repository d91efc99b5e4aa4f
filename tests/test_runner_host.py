"""Host side of the experiment runner (no GPU): the index stream of `DeviceLoader`, the dataset table, the metadata and
split sizes of the two dataset forms against fixtures produced by RUNNING the reference's loaders
(tests/golden/make_runner_golden.py), the command line, and argument validation of the new entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import runner_case as RC  # noqa: E402


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "runner_vectors.npz"), allow_pickle=False)


class _IndexDataset:
    """`batch` hands back its indices: what `DeviceLoader` yields is then its index stream."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def batch(self, indices, out=None):
        assert out is None
        return list(indices)


def _two_epochs(make, explicit_generator, unpack):
    """Index batches of two epochs after torch.manual_seed(42), len(), and a draw from the global RNG afterwards."""
    torch.manual_seed(42)
    loader = make(torch.Generator().manual_seed(5) if explicit_generator else None)
    epochs = [[[int(v) for v in unpack(b)] for b in loader] for _ in range(2)]
    return epochs, len(loader), torch.rand(1).item()


@pytest.mark.parametrize("batch_size", [1, 4])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("explicit_generator", [False, True])
def test_device_loader_index_stream_is_torchs(batch_size, drop_last, explicit_generator):
    from torch.utils.data import DataLoader, TensorDataset

    from graphcast_lite_amd.data import DeviceLoader

    n = 11
    want = _two_epochs(lambda g: DataLoader(TensorDataset(torch.arange(n)), batch_size=batch_size, shuffle=True,
                                            drop_last=drop_last, generator=g), explicit_generator, lambda b: b[0])
    got = _two_epochs(lambda g: DeviceLoader(_IndexDataset(n), batch_size=batch_size, shuffle=True, drop_last=drop_last,
                                             generator=g), explicit_generator, lambda b: b)
    assert got[0] == want[0]
    assert got[1] == want[1] == (n // batch_size if drop_last else -(-n // batch_size))
    assert got[2] == want[2]  # the same draws were taken from the global RNG
    assert got[0][0] != got[0][1]  # a fresh permutation per epoch
    seen = sorted(i for b in got[0][0] for i in b)
    assert len(seen) == len(set(seen)) == (n // batch_size * batch_size if drop_last else n)


def test_device_loader_fills_fitting_buffers_only():
    from graphcast_lite_amd.data import DeviceLoader

    class Shaped(_IndexDataset):
        def batch_shapes(self, B):
            return (B, 3, 4), (B, 3, 2)

        def batch(self, indices, out=None):
            return len(indices), out

    bufs = (torch.zeros(4, 3, 4), torch.zeros(4, 3, 2))
    got = list(DeviceLoader(Shaped(10), batch_size=4, buffers=lambda: bufs))
    assert [b for b, _ in got] == [4, 4, 2]
    assert got[0][1] is not None and got[0][1][0] is bufs[0] and got[1][1][1] is bufs[1]
    assert got[2][1] is None  # the short last batch does not fit
    assert all(o is None for _, o in DeviceLoader(Shaped(10), batch_size=4, buffers=lambda: None))


def test_dataset_table_matches_reference(z):
    from graphcast_lite_amd.data import DatasetMetadata, get_dataset_metadata

    assert len(z["table_names"]) == 9
    for name, row in zip(z["table_names"], z["table_values"]):
        m = get_dataset_metadata(str(name))
        assert isinstance(m, DatasetMetadata)
        assert [int(m.flattened), m.num_latitudes, m.num_longitudes, m.num_features, m.obs_window, m.pred_window] == list(row)
        assert m.flat_grid is False and m.num_grid_nodes == row[1] * row[2] and m.is_regional is None
    for bad in (str(z["table_unknown"]), "no_such_dataset"):
        with pytest.raises(NotImplementedError):
            get_dataset_metadata(bad)


@pytest.mark.parametrize("kind", ["reg", "flat"])
def test_chunked_metadata_and_split_lengths_match_reference(kind, z, tmp_path):
    """`load_chunked_datasets` on the host (device="cpu" uploads nothing and launches nothing)."""
    from graphcast_lite_amd.data import chunked_metadata, load_chunked_datasets

    path = RC.write_chunked(str(tmp_path / kind), z, flat=kind == "flat")
    train, val, test, md = load_chunked_datasets(path, obs_window=RC.CH_OBS, pred_steps=RC.CH_PRED,
                                                 n_features=RC.CH_FEAT, device="cpu")
    assert [len(train), len(val), len(test)] == list(z[f"chk_{kind}_len"])
    assert (train.split, val.split, test.split) == ("train", "val", "test_only")
    assert train.chunks[0].data_ptr() == val.chunks[0].data_ptr() == test.chunks[0].data_ptr()
    for m in (md, chunked_metadata(path, RC.CH_OBS, RC.CH_PRED, RC.CH_FEAT)[0]):
        got = [int(m.flattened), m.num_latitudes, m.num_longitudes, m.num_features, m.obs_window, m.pred_window,
               int(m.flat_grid), m.num_grid_nodes]
        assert got == list(z[f"chk_{kind}_meta"])
        for a, b in zip(m.cordinates, (z[f"chk_{kind}_lats"], z[f"chk_{kind}_lons"])):
            assert a.dtype == np.float32 and np.array_equal(a, b)
        if kind == "flat":
            assert np.array_equal(m.is_regional, z["chk_flat_is_regional"])
        else:
            assert m.is_regional is None
    # without n_features the variable list decides
    assert chunked_metadata(path)[1] == z[f"{kind}_series"].shape[-1]


def _table(monkeypatch):
    from graphcast_lite_amd import data

    monkeypatch.setitem(data._DATASETS, RC.NAME, RC.TABLE_ROW)
    return data


@pytest.mark.parametrize("tag,five_d,coords", [("ref4", False, False), ("ref5", True, True)])
def test_legacy_loader_host_part_matches_reference(tag, five_d, coords, z, tmp_path, monkeypatch):
    data = _table(monkeypatch)
    path = RC.write_legacy(str(tmp_path / tag), z, five_d=five_d, coords=coords)
    Xtr, ytr, Xte, yte, md = data.read_legacy_tensors(path, RC.data_config())
    assert [md.num_longitudes, md.num_latitudes] == list(z[f"{tag}_grid"]) == [RC.LON, RC.LAT]  # not the table's 64 x 32
    lats, lons = md.cordinates
    assert lats.dtype == lons.dtype == np.float32
    assert np.array_equal(lats, z[f"{tag}_lats"]) and np.array_equal(lons, z[f"{tag}_lons"])
    if not coords:
        assert lats[0] == -90 and lats[-1] == 90 and lons[0] == 0 and lons[-1] == 300
    G = RC.LON * RC.LAT
    assert tuple(Xtr.shape) == (RC.N_TRAIN, G, RC.OBS, RC.F) and tuple(yte.shape) == (RC.N_TEST, G, RC.PRED, RC.F)
    # the selection the kernel does, restated with torch on the host, against the reference's tensors
    n_val, n_test = data.legacy_split_sizes(RC.N_TEST)
    assert (n_val, n_test) == (2, 3) == (len(z[f"{tag}_X_val"]), len(z[f"{tag}_X_test"]))

    def sel(t, W, Wu):
        return t[:, :, W - Wu:, :RC.F_USED].reshape(t.shape[0], G, Wu * RC.F_USED).numpy()

    assert np.array_equal(sel(Xtr, RC.OBS, RC.OBS_USED), z[f"{tag}_X_train"])
    assert np.array_equal(sel(ytr, RC.PRED, RC.PRED_USED), z[f"{tag}_y_train"])
    assert np.array_equal(sel(Xte, RC.OBS, RC.OBS_USED)[:n_val], z[f"{tag}_X_val"])
    assert np.array_equal(sel(yte, RC.PRED, RC.PRED_USED)[n_val:], z[f"{tag}_y_test"])


def test_legacy_loader_shape_checks_raise(z, tmp_path, monkeypatch):
    data = _table(monkeypatch)
    path = RC.write_legacy(str(tmp_path / "d"), z)
    cfg = RC.data_config()
    for field in ("num_features_used", "obs_window_used", "pred_window_used"):
        bad = RC.data_config()
        setattr(bad, field, 9)
        with pytest.raises(AssertionError):
            data.read_legacy_tensors(path, bad)
    torch.save(torch.zeros(RC.N_TRAIN, RC.LON, RC.LAT, RC.OBS * RC.F + 1), os.path.join(path, "X_train.pt"))
    with pytest.raises(AssertionError):
        data.read_legacy_tensors(path, cfg)
    torch.save(torch.zeros(RC.N_TRAIN, RC.LON, RC.LAT, RC.OBS + 1, RC.F), os.path.join(path, "X_train.pt"))
    torch.save(torch.zeros(RC.N_TRAIN, RC.LON, RC.LAT, RC.PRED, RC.F), os.path.join(path, "y_train.pt"))
    with pytest.raises(AssertionError):
        data.read_legacy_tensors(path, cfg)
    torch.save(torch.zeros(RC.N_TRAIN, RC.LON * RC.LAT, RC.OBS * RC.F), os.path.join(path, "X_train.pt"))
    with pytest.raises(RuntimeError, match="ndim=3"):
        data.read_legacy_tensors(path, cfg)
    cfg.dataset_name = "no_such_dataset"
    with pytest.raises(NotImplementedError):
        data.read_legacy_tensors(path, cfg)


def test_weather_dataset_checks_indices_on_the_host():
    from graphcast_lite_amd.data import WeatherDataset

    ds = WeatherDataset(torch.zeros(5, 4, 3, 2), torch.zeros(5, 4, 1, 2), 2, 3, 2, 1, 2)
    assert len(ds) == 3 and ds.batch_shapes(2) == ((2, 4, 4), (2, 4, 2))
    for bad in ([3], [-1], [0, 1, 7]):
        with pytest.raises(ValueError, match="outside"):
            ds.batch(bad)
    with pytest.raises(ValueError):
        WeatherDataset(torch.zeros(5, 4, 3, 2), torch.zeros(5, 4, 1, 2), 3, 3, 2, 1, 2)


def test_cli_argument_handling(capsys):
    from graphcast_lite_amd import main as M

    assert M.parse_args(["exp"]) == ("exp", False, None)
    assert M.parse_args(["exp", "--resume"]) == ("exp", True, None)
    assert M.parse_args(["exp", "--pretrained", "m.pth", "--resume"]) == ("exp", True, "m.pth")
    with pytest.raises(SystemExit) as e:
        M.main(["--help"])
    assert e.value.code == 0 and "usage:" in capsys.readouterr().out
    for bad in ([], ["--resume"], ["exp", "--pretrained"]):
        with pytest.raises(SystemExit) as e:
            M.main(bad)
        assert e.value.code == 2 and "usage:" in capsys.readouterr().err


def test_cli_without_arguments_exits_with_usage():
    r = subprocess.run([sys.executable, "-m", "graphcast_lite_amd.main"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "usage: python -m graphcast_lite_amd.main" in r.stderr


def test_seeds_are_always_42():
    import random

    from graphcast_lite_amd.main import set_random_seeds

    set_random_seeds(7)
    a = (random.random(), np.random.rand(), torch.rand(1).item())
    set_random_seeds(42)
    assert a == (random.random(), np.random.rand(), torch.rand(1).item())


def test_region_detection():
    from graphcast_lite_amd.main import detect_region_bounds

    assert detect_region_bounds(None) is None
    assert detect_region_bounds((np.linspace(-90, 90, 8), np.linspace(0, 315, 8))) is None
    assert detect_region_bounds((np.linspace(50, 62, 4), np.linspace(0, 315, 8))) is None
    assert detect_region_bounds((np.linspace(50, 62, 4), np.linspace(80, 100, 6))) == (50.0, 62.0, 80.0, 100.0)


def test_new_entry_points_validate_before_any_hip_call(lib_built):
    L = lib_built
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ws = L.gcl_eval_colstats_ws_bytes(2, 48, 5)
    assert ws == 2 * 5 * 7 * 1 * 8 and L.gcl_eval_colstats_ws_bytes(2, 2051, 19) == 2 * 19 * 7 * 33 * 8
    assert L.gcl_eval_colstats_ws_bytes(0, 48, 5) == 0

    def colstats(delta=p, x_last=p, y=p, stats=p, G=4, ws_p=p, ws_bytes=1 << 20):
        return L.gcl_eval_colstats(delta, 1, 4, x_last, 1, 4, y, 1, 4, None, None, 1, None, 0, 0, stats, 1, G, 1, ws_p,
                                   ws_bytes, None)

    assert colstats(G=1) == -1 and b"at least 2 nodes" in L.gcl_last_error()
    for kw in (dict(delta=None), dict(x_last=None), dict(y=None), dict(stats=None)):
        assert colstats(**kw) == -1 and b"null argument" in L.gcl_last_error()
    assert colstats(ws_p=None) == -1 and b"workspace" in L.gcl_last_error()
    assert colstats(ws_bytes=8) == -1 and b"workspace" in L.gcl_last_error()
    assert L.gcl_eval_accumulate(None, None, None, 1.0, 1, 4, 1, p, None) == -1 and b"null argument" in L.gcl_last_error()
    assert L.gcl_eval_accumulate(p, None, None, 1.0, 1, 1, 1, p, None) == -1 and b"at least 2 nodes" in L.gcl_last_error()

    def pack(X=p, idx=p, out=p, Wx=3, Wxu=2, Y=None, outY=None, Wy=0, Wyu=0, F=5, Fu=3, ldx=6):
        return L.gcl_tensor_batch_pack(X, Wx, Wxu, Y, Wy, Wyu, 4, 2, F, Fu, idx, 1, out, ldx, 12, outY, 0, 0, None)

    assert pack(Wxu=4) == -1 and b"4 of 3 stored steps" in L.gcl_last_error()
    assert pack(Y=p, outY=p, Wy=1, Wyu=2) == -1 and b"2 of 1 stored steps" in L.gcl_last_error()
    assert pack(Fu=6) == -1 and b"6 of 5 features" in L.gcl_last_error()
    assert pack(ldx=5) == -1 and b"row too short" in L.gcl_last_error()
    assert pack(Y=p) == -1 and b"go together" in L.gcl_last_error()
    for kw in (dict(X=None), dict(idx=None), dict(out=None)):
        assert pack(**kw) == -1 and b"null argument" in L.gcl_last_error()
