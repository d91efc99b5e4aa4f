"""Observation files for data assimilation: the counterparts of `scripts/create_obs.py` and
`scripts/generate_assim_dataset.py`, whose output `python -m graphcast_lite_amd.predict --obs-path` reads.

* `sparse_observations`: a truth tensor [B, G, P*C] on the device -> the same shape with NaN everywhere but at the
  station rows and the observed channels, one launch (`gcl_obs_pack`).  The predict loop forms its inline observations
  (`scripts/predict.py:471-483`) with it, batch by batch, and `create_obs` the whole file.
* `create_obs` (`scripts/create_obs.py:8-148`): the second half of `y_test.pt` (the test split of the legacy loader), the
  station draw, the variable lookup, the `[N, G, P*C]` file.
* `generate_assim_dataset` (`scripts/generate_assim_dataset.py:43-123`): `y_obs.pt`, `mask_flat.pt`, `meta.json` in a
  subfolder of the experiment directory.  Host only.

`python -m graphcast_lite_amd.observations create ...` / `... package ...` take the two scripts' options.

Kernel: csrc/predict.hip.
"""
import argparse
import json
import os
import sys
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip

_MASKS = {}


def _mask_u8(flags: np.ndarray, device) -> torch.Tensor:
    """A small uint8 mask on the device, uploaded once per distinct content (captured launches keep pointing at it)."""
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    key = (flags.tobytes(), str(device))
    t = _MASKS.get(key)
    if t is None:
        t = torch.from_numpy(flags.copy()).to(device)
        _MASKS[key] = t
    return t


def station_mask(station_rows, G: int, device) -> torch.Tensor:
    """uint8 [G] on the device: 1 at the station rows (any order, repeats allowed).  A uint8 device tensor of G entries
    is taken as the mask itself."""
    if isinstance(station_rows, torch.Tensor) and station_rows.dtype == torch.uint8 and station_rows.is_cuda:
        if station_rows.numel() != G:
            raise ValueError(f"station mask of {station_rows.numel()} entries for {G} nodes")
        return station_rows
    rows = (station_rows.detach().cpu().numpy() if isinstance(station_rows, torch.Tensor) else np.asarray(station_rows))
    rows = rows.astype(np.int64).reshape(-1)
    if rows.size and (rows.min() < 0 or rows.max() >= G):
        raise ValueError(f"station row outside [0, {G})")
    flags = np.zeros(G, dtype=np.uint8)
    flags[rows] = 1
    return _mask_u8(flags, device)


def channel_mask(channels, C: Optional[int], device) -> torch.Tensor:
    """uint8 [C] on the device: 1 at the observed channels.  channels None: every channel (C may then be None: one
    entry that every column maps to)."""
    if channels is None:
        return _mask_u8(np.ones(1 if C is None else int(C), dtype=np.uint8), device)
    if C is None:
        raise ValueError("sparse_observations: num_channels is needed with a channel list")
    idx = np.asarray(list(channels), dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= C):
        raise ValueError(f"observed channel outside [0, {C})")
    flags = np.zeros(int(C), dtype=np.uint8)
    flags[idx] = 1
    return _mask_u8(flags, device)


def sparse_observations(y: torch.Tensor, station_rows, channels: Optional[Sequence[int]] = None,
                        out: Optional[torch.Tensor] = None, num_channels: Optional[int] = None) -> torch.Tensor:
    """y [B, G, P*C] (or [G, P*C]) float32 on the device -> the same shape: y at (station row, observed channel), NaN
    elsewhere.  station_rows: grid indices (or a uint8 device mask [G]); channels: observed channel indices of the
    `num_channels` channels a step holds (None: all).  out may be y (in place).  One launch, no host read."""
    squeeze = y.dim() == 2
    y3 = y.unsqueeze(0) if squeeze else y
    if y3.dim() != 3:
        raise ValueError(f"sparse_observations: expected [B, G, P*C] or [G, P*C], got {tuple(y.shape)}")
    if y3.stride(2) != 1:
        y3 = y3.contiguous()
    o3 = None
    if out is not None:
        o3 = out.unsqueeze(0) if squeeze else out
    res = hip.obs_pack(y3, station_mask(station_rows, y3.shape[1], y3.device),
                       channel_mask(channels, num_channels, y3.device), o3)
    return res[0] if squeeze else res


# ======================================================================================================================
# scripts/create_obs.py
# ======================================================================================================================
def flatten_targets(y_full: torch.Tensor, C: int):
    """The layouts `create_obs.py:49-75` accepts, as (N, G, P): [N, G, P*C], [N, lon, lat, P*C] and [N, lon, lat, P, C]
    (the script's fourth branch, [N, G, P, C'] with C' no multiple of the variable count, cannot pass its own final
    reshape and is refused here)."""
    shape = tuple(y_full.shape)
    if len(shape) == 3:
        N, G, PC = shape
        return N, G, PC // C
    if len(shape) == 4 and shape[-1] % C == 0:
        N, lon, lat, PC = shape
        return N, lon * lat, PC // C
    if len(shape) == 5 and shape[-1] == C:
        N, lon, lat, P, _ = shape
        return N, lon * lat, P
    raise ValueError(f"create_obs: cannot read targets of shape {shape} with {C} variables")


def roi_candidates(roi, coords_path, G: int) -> np.ndarray:
    """`create_obs.py:87-104`: the nodes inside (lat_min, lat_max, lon_min, lon_max), from per-node coordinates when
    coords.npz holds G of them, else from the axes meshed as `np.meshgrid(lons, lats)` (the script's order)."""
    lat_min, lat_max, lon_min, lon_max = roi
    coords = np.load(coords_path)
    c_lats = coords["latitude"].astype(np.float32)
    c_lons = coords["longitude"].astype(np.float32)
    if c_lats.ndim == 1 and len(c_lats) == G:
        inside = (c_lats >= lat_min) & (c_lats <= lat_max) & (c_lons >= lon_min) & (c_lons <= lon_max)
    else:
        lon_grid, lat_grid = np.meshgrid(c_lons, c_lats)
        la, lo = lat_grid.ravel(), lon_grid.ravel()
        inside = (la >= lat_min) & (la <= lat_max) & (lo >= lon_min) & (lo <= lon_max)
    return np.where(inside)[0]


def draw_stations(candidates: np.ndarray, sparsity: float, seed: int) -> np.ndarray:
    """`create_obs.py:83,108-111`: max(1, int(n * sparsity)) of the candidates without replacement from a generator
    seeded with `seed` (the stream of `np.random.seed(seed); np.random.choice(...)`), in the order drawn."""
    n = int(len(candidates) * sparsity)
    if n == 0:
        n = 1
    return np.random.RandomState(seed).choice(candidates, n, replace=False)


def variable_indices(var_names: Sequence[str], wanted: str, say=print) -> Optional[list]:
    """`create_obs.py:115-137`: 'all' -> every index; else the indices of the comma-separated names, unknown names
    reported and left out.  None when nothing is left."""
    if wanted == "all":
        return list(range(len(var_names)))
    idx = []
    for v in (s.strip() for s in wanted.split(",")):
        if v in var_names:
            idx.append(list(var_names).index(v))
        else:
            say(f"[WARN] variable '{v}' not found; available: {list(var_names)}")
    return idx or None


def create_obs(y_path, vars_path, save_path, sparsity: float = 0.1, vars: str = "all", seed: int = 42, roi=None,
               coords_path=None, device=None, say=print):
    """`scripts/create_obs.py`: writes the sparse observation tensor [N, G, P*C] (NaN = not observed) of the test half
    of `y_path` to `save_path` and returns it (on the host), or None where the script gives up (no coordinates for
    `roi`, no known variable).  The masking runs on the device in one launch."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("create_obs needs a GPU (the HIP path has no CPU fallback)")
        device = "cuda:0"
    say(f"Loading {y_path} ...")
    y_full = torch.load(str(y_path), map_location="cpu", weights_only=True)
    total = y_full.shape[0]
    val_size = total // 2  # the legacy loader's validation half (src/data/dataloader.py:142-147)
    say(f"[SPLIT] {total} samples in the file: the first {val_size} (validation) are dropped, the last "
        f"{total - val_size} (test) kept")
    y_full = y_full[val_size:]
    with open(vars_path) as fh:
        var_names = json.load(fh)
    C = len(var_names)
    N, G, P = flatten_targets(y_full, C)
    say(f"N={N}, G={G}, steps={P}, variables={C}")
    candidates = np.arange(G)
    if roi is not None:
        if coords_path is None:
            say("ERROR: --roi needs --coords-path (coords.npz)")
            return None
        candidates = roi_candidates(roi, coords_path, G)
        say(f"[ROI] {len(candidates)} nodes inside [{roi[0]:.0f}-{roi[1]:.0f}N, {roi[2]:.0f}-{roi[3]:.0f}E]")
    stations = draw_stations(candidates, sparsity, seed)
    say(f"{len(stations)} stations drawn from {len(candidates)} nodes ({sparsity * 100}%)")
    idx = variable_indices(var_names, vars, say=say)
    if idx is None:
        say("ERROR: no variable selected; check the names")
        return None
    say("All variables are observed." if vars == "all" else f"Observed variable indices: {idx}")
    y3 = y_full.reshape(N, G, P * C).to(torch.float32).to(device)
    obs = sparse_observations(y3, stations, channels=idx, num_channels=C, out=y3).cpu()
    if os.path.dirname(str(save_path)):
        os.makedirs(os.path.dirname(str(save_path)), exist_ok=True)
    torch.save(obs, str(save_path))
    say(f"Saved {save_path}")
    return obs


# ======================================================================================================================
# scripts/generate_assim_dataset.py
# ======================================================================================================================
def load_feature_list(path) -> Optional[list]:
    """`generate_assim_dataset.py:22-41`: a JSON list, or text with one name per line or comma-separated names; None
    when the file is absent, empty or unreadable."""
    if not path:
        return None
    p = Path(path)
    if not p.exists():
        return None
    try:
        if p.suffix.lower() in (".json", ".jsn"):
            return json.loads(p.read_text())
        txt = p.read_text().strip()
        if not txt:
            return None
        if "\n" in txt and "," not in txt:
            return [t.strip() for t in txt.splitlines() if t.strip()]
        return [t.strip() for t in txt.split(",") if t.strip()]
    except Exception:
        return None


def generate_assim_dataset(experiment_dir, vars: str = "", feature_list: str = "", indices: str = "",
                           out_name: str = "assimilation", say=print) -> dict:
    """`scripts/generate_assim_dataset.py`: `<experiment_dir>/<out_name>/{y_obs.pt, mask_flat.pt, meta.json}` from
    `<experiment_dir>/y_test.pt` ([N, lon, lat, P, C], or [N, G, P*C] with the horizon read from config.json) and the
    variables to assimilate (names through the feature list, or indices; none given: all).  Returns the meta
    dictionary."""
    from .train import FileNames

    exp = Path(experiment_dir)
    y_path = exp / FileNames.TEST_Y
    if not y_path.exists():
        raise SystemExit(f"Not found: {y_path}")
    y_test = torch.load(str(y_path), map_location="cpu", weights_only=True)
    if y_test.dim() == 5:
        N, LON, LAT, P_used, C_total = y_test.shape
        y_flat = y_test.reshape(N, LON * LAT, P_used * C_total).contiguous()
    elif y_test.dim() == 3:
        data_cfg = json.loads((exp / "config.json").read_text()).get("data", {})
        P_used = int(data_cfg.get("pred_window_used", data_cfg.get("pred_window", 1)))
        C_total = y_test.shape[2] // P_used
        y_flat = y_test
    else:
        raise SystemExit(f"Unexpected y_test shape: {tuple(y_test.shape)}")
    P_used, C_total = int(P_used), int(C_total)
    feature_names = load_feature_list(feature_list) if feature_list else load_feature_list(str(exp / "features.json"))
    var_names = [v.strip() for v in vars.split(",") if v.strip()]
    if var_names and not feature_names:
        say("[WARN] variable names given but no feature list found: names cannot be mapped to indices, the mask selects "
            "every variable.  Consider --feature-list or --indices.")
        chosen = []
    elif var_names:
        where = {n: i for i, n in enumerate(feature_names)}
        chosen = []
        for vn in var_names:
            if vn not in where:
                say(f"[WARN] variable {vn} not in feature list; skipping")
                continue
            chosen.append(where[vn])
    else:
        chosen = [int(s) for s in indices.split(",") if s.strip().isdigit()]
    if not chosen:
        chosen = list(range(C_total))
    mask = torch.zeros(C_total, dtype=torch.bool)
    for i in chosen:
        if 0 <= i < C_total:
            mask[i] = True
    outdir = exp / out_name
    outdir.mkdir(parents=True, exist_ok=True)
    torch.save(y_flat, str(outdir / "y_obs.pt"))
    torch.save(mask.repeat(P_used), str(outdir / "mask_flat.pt"))
    meta = {
        "feature_list_used": feature_names,
        "vars_requested": var_names,
        "indices_used": chosen,
        "pred_window": P_used,
        "num_features": C_total,
        "y_shape": list(y_flat.shape),
        "notes": "y_obs.pt has shape [N, G, P*C]; mask_flat.pt length = P*C (booleans).",
    }
    (outdir / "meta.json").write_text(json.dumps(meta, ensure_ascii=False, indent=2))
    say(f"Saved: {outdir / 'y_obs.pt'}; {outdir / 'mask_flat.pt'}")
    say(json.dumps(meta, ensure_ascii=False, indent=2))
    return meta


# ======================================================================================================================
# Command line
# ======================================================================================================================
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m graphcast_lite_amd.observations")
    sub = ap.add_subparsers(dest="command", required=True)
    c = sub.add_parser("create", help="scripts/create_obs.py")
    c.add_argument("--y-path", type=str, required=True)
    c.add_argument("--vars-path", type=str, required=True)
    c.add_argument("--save-path", type=str, required=True)
    c.add_argument("--sparsity", type=float, default=0.1)
    c.add_argument("--vars", type=str, default="all")
    c.add_argument("--seed", type=int, default=42)
    c.add_argument("--roi", nargs=4, type=float, default=None, metavar=("LAT_MIN", "LAT_MAX", "LON_MIN", "LON_MAX"))
    c.add_argument("--coords-path", type=str, default=None)
    p = sub.add_parser("package", help="scripts/generate_assim_dataset.py")
    p.add_argument("experiment_dir", type=str)
    p.add_argument("--vars", type=str, default="")
    p.add_argument("--feature-list", type=str, default="")
    p.add_argument("--indices", type=str, default="")
    p.add_argument("--out-name", type=str, default="assimilation")
    return ap


def main(argv=None, device=None):
    a = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    if a.command == "create":
        return create_obs(a.y_path, a.vars_path, a.save_path, sparsity=a.sparsity, vars=a.vars, seed=a.seed, roi=a.roi,
                          coords_path=a.coords_path, device=device)
    return generate_assim_dataset(a.experiment_dir, vars=a.vars, feature_list=a.feature_list, indices=a.indices,
                                  out_name=a.out_name)


if __name__ == "__main__":
    main()
