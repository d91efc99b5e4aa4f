"""Generate the live-forecast fixtures by RUNNING the reference's own `scripts/live_gdas_forecast.py` and
`scripts/export_live_runtime_bundle.py` (numpy, scipy).

Run from the repo root, only where the reference checkout (`make_golden.REF`) and scipy exist (never on the GPU box):

    python tests/golden/make_live_golden.py

`xarray` is absent from this image and gets an inert placeholder in `sys.modules`; the reference's functions are handed
the small stand-in `Field` / `Group` below, which offer only what they touch (`.coords`, `.dims`, `.values`, `[name]`,
`.data_vars`, `.sel`).

Output (data only - arrays and recorded text, no reference source text): tests/golden/live_vectors.npz
  node_lat, node_lon    the 700 query nodes (690 seeded over the sphere + the edge cases)
  interp_<name>         `interp_to_nodes` of every field of cycle 0 (key: the variable name with @ -> _)
  input_tensor          the normalised [G, obs * C] window of the two cycles (main():612-620)
  warnings              the warning strings of both cycles, prefixed as main() prefixes them
  x_mean, x_std         the scalers used
  static_z_surf / lsm   the template statics
  summary_city / summary_empty   `summarize_city`'s text for a synthetic [G, 4, C] forecast with a non-empty / empty
                        city box; city_lat / city_lon the coordinates of the non-empty case
  bundle_<kind>_files, bundle_<kind>_meta, assets_<kind>_*   the file listing, bundle_meta.json text and the arrays of
                        `export_bundle` -> `load_runtime_assets` on a tiny flat / regular dataset
The source fields come from `field_values()` below (seeded numpy), which tests/test_live.py restates.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types
from datetime import datetime, timedelta, timezone
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (where the reference checkout lives)

REF = make_golden.REF

VAR_ORDER = ["t2m", "10u", "10v", "msl", "tp", "sp", "tcwv", "z_surf", "lsm",
             "t@850", "u@850", "v@850", "z@850", "q@850", "t@500", "u@500", "v@500", "z@500", "q@500",
             "sst", "cape"]  # DEFAULT_VAR_ORDER + two names outside var_specs
ABSENT = ("tp", "q@850", "q@500")  # tp, and the whole isobaric q group (one level alone cannot be absent)
SURFACE_B = ("tcwv",)  # the second variable group: a 19 x 36 grid
CAPPED = ("sp",)  # the third: stops at +-75 deg, so the polar nodes extrapolate
OBS = 2
T0 = datetime(2024, 2, 28, 18, tzinfo=timezone.utc)
SUMMARY_SEED = 90453  # the first seed whose 48 printed numbers all keep the margin asserted in main()


def axes(kind):
    """(lats, lons) of the source grids, float64 as a decoder would hand them over."""
    if kind == "a":  # 13 x 24, 15 deg: latitudes descending, longitudes -180 .. 165
        return np.linspace(90.0, -90.0, 13), -180.0 + 15.0 * np.arange(24)
    if kind == "b":  # 19 x 36, 10 deg, ascending latitudes, longitudes 0 .. 350
        return np.linspace(-90.0, 90.0, 19), 10.0 * np.arange(36)
    return np.linspace(75.0, -75.0, 11), 20.0 * np.arange(18) - 100.0  # "c": 11 x 18, +-75 deg, -100 .. 240


def kind_of(name):
    return "b" if name in SURFACE_B else "c" if name in CAPPED else "a"


def field_values(name, cycle):
    """Seeded float32 field of a variable in physical units, in its grid's own orientation."""
    lats, lons = axes(kind_of(name))
    rng = np.random.default_rng(1000 * cycle + VAR_ORDER.index(name))
    x = rng.standard_normal((lats.size, lons.size))
    if name in ("msl", "sp"):
        x = 100000.0 + 1500.0 * x
    elif name.startswith("t"):
        x = 270.0 + 12.0 * x
    elif name.startswith("z"):
        x = 30000.0 + 800.0 * x
    elif name.startswith("q"):
        x = 1e-3 * np.abs(x)
    else:
        x = 7.0 * x
    return x.astype(np.float32)


def nodes():
    rng = np.random.default_rng(42)
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, 690)))
    lon = rng.uniform(0, 360, 690)
    lat = np.concatenate([lat, [90.0, -90.0, 10.0, 20.0, 30.0, -40.0, 80.0, -85.0, 75.0, -75.0]])
    lon = np.concatenate([lon, [123.0, 321.0, 0.0, 359.99, 360.0 - 1e-4, -77.5, 200.0, 15.0, 240.0, 250.0]])
    return lat.astype(np.float32), lon.astype(np.float32)


def scalers():
    rng = np.random.default_rng(5)
    mean = rng.normal(0, 50, len(VAR_ORDER) + 2).astype(np.float32)  # (longer than var_order: main() slices them)
    std = rng.uniform(0.5, 40, len(VAR_ORDER) + 2).astype(np.float32)
    return mean, std


def statics(G):
    rng = np.random.default_rng(6)
    return {"z_surf": (500.0 * np.abs(rng.standard_normal(G))).astype(np.float32),
            "lsm": (rng.random(G) < 0.3).astype(np.float32)}


def summary_case(G, C):
    """Synthetic physical forecast [G, 4, C] and per-node coordinates with some nodes inside the city box."""
    rng = np.random.default_rng(SUMMARY_SEED)
    pred = rng.standard_normal((G, 4, C))
    pred[..., 0] = 263.0 + 9.0 * pred[..., 0]
    pred[..., 1:3] *= 5.0
    pred[..., 3] = 1012.0 + 11.0 * pred[..., 3]
    lat = rng.uniform(54.0, 58.0, G).astype(np.float32)
    lon = rng.uniform(90.0, 96.0, G).astype(np.float32)
    return pred.astype(np.float32), lat, lon


# ----------------------------------------------------------------------------------------------------------------------
# what the reference touches of xarray
# ----------------------------------------------------------------------------------------------------------------------
class Coord:
    def __init__(self, values):
        self.values = values


class Field:
    def __init__(self, values, lats, lons, levels=None):
        self.values = values
        self.coords = {"latitude": Coord(lats), "longitude": Coord(lons)}
        self.dims = ("latitude", "longitude")
        self._levels = levels
        if levels is not None:
            self.coords["isobaricInhPa"] = Coord(np.array(sorted(levels)))
            self.dims = ("isobaricInhPa",) + self.dims

    def __getitem__(self, name):
        return self.coords[name]

    def sel(self, sel):
        (name, level), = sel.items()
        assert name == "isobaricInhPa"
        return self._levels[level]


class Group:
    def __init__(self, **data_vars):
        self.data_vars = data_vars

    def __getitem__(self, name):
        return self.data_vars[name]


GROUPS = {"t2m": ("t2m", "2t"), "10u": ("10u", "10u"), "10v": ("10v", "10v"), "msl": ("msl", "prmsl"),
          "sp": ("sp", "sp"), "tcwv": ("tcwv", "pwat"), "tp": ("tp", "tp")}
ISOBARIC = {"t": "t", "u": "u", "v": "v", "z": "gh", "q": "q"}


def payload(cycle):
    """The dict of groups `open_gdas_payload` would return for the fields of `cycle` (ABSENT left out)."""
    out = {}
    for name, (group, short) in GROUPS.items():
        if name not in ABSENT:
            out[group] = Group(**{short: Field(field_values(name, cycle), *axes(kind_of(name)))})
    for v, short in ISOBARIC.items():
        levels = {p: Field(field_values(f"{v}@{p}", cycle), *axes("a")) for p in (850, 500)
                  if f"{v}@{p}" not in ABSENT}
        if levels:
            out[f"isobaric_{v}"] = Group(**{short: Field(None, *axes("a"), levels=levels)})
    return out


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference():
    make_golden._placeholders()
    sys.modules.setdefault("xarray", types.ModuleType("xarray"))
    sys.modules["xarray"].Dataset = sys.modules["xarray"].DataArray = object
    sys.path.insert(0, REF)
    live = _load(os.path.join(REF, "scripts", "live_gdas_forecast.py"), "_ref_live")
    export = _load(os.path.join(REF, "scripts", "export_live_runtime_bundle.py"), "_ref_export")
    return live, export


def tiny_dataset(folder: Path, flat: bool):
    """A dataset directory as the builders leave it: 3 frames, 5 variables, 12 nodes (flat) or 4 x 3 (lon, lat)."""
    rng = np.random.default_rng(11 + flat)
    names = ["t2m", "z_surf", "msl", "lsm", "10u"]
    folder.mkdir(parents=True)
    shape = (3, 12, 5) if flat else (3, 4, 3, 5)
    (rng.standard_normal(shape) * 100).astype(np.float16).tofile(folder / "data.npy")
    info = {"n_time": 3, "n_feat": 5, "variables": names}
    info.update({"flat": True, "n_nodes": 12} if flat else {"n_lon": 4, "n_lat": 3})
    (folder / "dataset_info.json").write_text(json.dumps(info))
    (folder / "variables.json").write_text(json.dumps(names))
    coords = {"latitude": rng.uniform(-90, 90, 12), "longitude": rng.uniform(0, 360, 12)}  # float64 on disk
    if flat:
        coords["is_regional"] = rng.random(12) < 0.5
        np.savez(folder / "scalers.npz", x_mean=rng.normal(size=5), x_scale=rng.uniform(1, 2, 5),
                 y_mean=rng.normal(size=5), y_scale=rng.uniform(1, 2, 5))
    else:
        np.savez(folder / "scalers.npz", mean=rng.normal(size=5), std=rng.uniform(1, 2, 5))
    np.savez(folder / "coords.npz", **coords)


def main():
    live, export = _reference()
    out = {}
    lat, lon = nodes()
    G, C = lat.size, len(VAR_ORDER)
    out["node_lat"], out["node_lon"] = lat, lon
    mean, std = scalers()
    out["x_mean"], out["x_std"] = mean, std
    st = statics(G)
    out["static_z_surf"], out["static_lsm"] = st["z_surf"], st["lsm"]

    # --- interp_to_nodes per variable, the window and the warnings, as main():612-620 forms them ----------------------
    cycles = [T0 + timedelta(hours=6 * k) for k in range(OBS)]
    frames, warnings = [], []
    for k, dt in enumerate(cycles):
        pl = payload(k)
        extracted, cw = live.extract_live_channels(pl, lat, lon, VAR_ORDER, st)
        warnings += [f"{dt.isoformat()}: {line}" for line in cw]
        frame = np.stack([extracted[n] for n in VAR_ORDER], axis=-1).astype(np.float32)
        frames.append(live.normalize_frame(frame, mean[:C], std[:C]))
        if k == 0:
            for name in VAR_ORDER:
                if name in live.DEFAULT_VAR_ORDER and name not in ABSENT and name not in st:
                    fld = Field(field_values(name, 0), *axes(kind_of(name)))
                    out["interp_" + name.replace("@", "_")] = live.interp_to_nodes(fld, lat, lon)
    out["input_tensor"] = np.stack(frames, axis=1).reshape(G, OBS * C).astype(np.float32)
    assert out["input_tensor"].dtype == np.float32 and np.isfinite(out["input_tensor"]).all()
    out["warnings"] = np.array(warnings)

    # --- summarize_city ------------------------------------------------------------------------------------------------
    pred, clat, clon = summary_case(G, C)
    out["city_lat"], out["city_lon"] = clat, clon
    with tempfile.TemporaryDirectory() as tmp:
        p = Path(tmp) / "summary.txt"
        live.summarize_city(p, pred, clat, clon, VAR_ORDER, cycles, warnings)
        out["summary_city"] = np.array(p.read_text(encoding="utf-8"))
        live.summarize_city(p, pred, lat, lon, VAR_ORDER, cycles, [])
        out["summary_empty"] = np.array(p.read_text(encoding="utf-8"))
    assert "City-area means:" in str(out["summary_city"]) and "City-area means:" not in str(out["summary_empty"])
    mask = live.build_city_mask(clat, clon)
    assert mask.sum() > 8
    # Every printed number lies more than 1e-3 from the nearest two-decimal rounding boundary (x.xx5), i.e. more than
    # 0.1 of the last printed digit, so the text cannot hinge on the last bit of a float32 mean (one ulp at 1012 hPa is
    # 6e-5).  A seed passes with probability 0.8^48, about 2e-5: SUMMARY_SEED is the first that does.
    worst = 1.0
    for s in range(4):
        for name in ("t2m", "10u", "10v", "msl"):
            v = pred[:, s, VAR_ORDER.index(name)][mask]
            v = v - 273.15 if name == "t2m" else v
            for x in (float(v.mean()), float(v.min()), float(v.max())):
                margin = abs(abs(x) * 100.0 % 1.0 - 0.5)
                worst = min(worst, margin)
                assert margin > 0.1, f"{name} step {s}: {x!r} sits on a rounding boundary; change SUMMARY_SEED"
    print(f"summary: smallest margin from a rounding boundary {worst / 100:.2e} (absolute)")

    # --- export_bundle -> load_runtime_assets --------------------------------------------------------------------------
    for kind, flat in (("flat", True), ("regular", False)):
        with tempfile.TemporaryDirectory() as tmp:
            data, bundle = Path(tmp) / "data", Path(tmp) / "bundle"
            tiny_dataset(data, flat)
            export.export_bundle(data, bundle)
            out[f"bundle_{kind}_files"] = np.array(sorted(q.name for q in bundle.iterdir()))
            out[f"bundle_{kind}_meta"] = np.array((bundle / "bundle_meta.json").read_text(encoding="utf-8"))
            out[f"bundle_{kind}_variables"] = np.array((bundle / "variables.json").read_text(encoding="utf-8"))
            for fn in ("coords.npz", "scalers.npz", "static_fields.npz"):
                z = np.load(bundle / fn)
                out[f"bundle_{kind}_{fn[:-4]}_keys"] = np.array(sorted(z.files))
                for key in z.files:
                    out[f"bundle_{kind}_{fn[:-4]}_{key}"] = z[key]
            for src, args in (("bundle", (None, bundle)), ("data", (data, None))):
                xm, xs, ym, ys, vo, la, lo, ts, meta = live.load_runtime_assets(*args, 2, 1)
                pre = f"assets_{kind}_{src}_"
                out.update({pre + "x_mean": xm, pre + "x_std": xs, pre + "y_mean": ym, pre + "y_std": ys,
                            pre + "var_order": np.array(vo), pre + "lat": la, pre + "lon": lo,
                            pre + "static_keys": np.array(sorted(ts)),
                            pre + "num_grid_nodes": np.int64(meta.num_grid_nodes),
                            pre + "flat_grid": np.bool_(meta.flat_grid),
                            pre + "has_is_regional": np.bool_(meta.is_regional is not None)})
                for key, v in ts.items():
                    out[pre + "static_" + key] = v
                if meta.is_regional is not None:
                    out[pre + "is_regional"] = meta.is_regional

    path = os.path.join(HERE, "live_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
