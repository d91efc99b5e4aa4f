"""Run an experiment directory end to end: `python -m graphcast_lite_amd.main <experiment_dir> [--resume] [--pretrained p]`.

The reference's entry point (`src/main.py:23-264`) on the HIP path: the dataset named by the configuration is loaded into
HBM (chunked fp16 series or the legacy `.pt` tensors), three `DeviceLoader`s hand out device batches, the model is built
with the regional mesh auto-detection, the fine-tuning optimiser comes from `build_optimizer`, and `train()` runs with the
fused validation step (`Evaluator`).
"""
import os
import random
import sys

import numpy as np
import torch

from .config import ExperimentConfig
from .data import (CHUNKED_DATASET_NAMES, DatasetMetadata, DeviceLoader, load_chunked_datasets,
                   load_train_and_test_datasets)
from .models import WeatherPrediction
from .train import Evaluator, FileNames, build_optimizer, loss_masks, train
from .utils import load_from_json_file

RESULTS_FOLDER = "results"  # src/constants.py FolderNames.RESULTS
USAGE = "usage: python -m graphcast_lite_amd.main <experiment_dir> [--resume] [--pretrained <model.pth>]"


def set_random_seeds(seed: int = 42):
    """src/main.py:23-26: the argument is ignored there as well, the seed is always 42."""
    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)


def load_model_from_experiment_config(experiment_config: ExperimentConfig, device, dataset_metadata: DatasetMetadata,
                                      coordinates=None, region_bounds=None, mesh_buffer: float = 15.0,
                                      flat_grid: bool = False) -> WeatherPrediction:
    """src/main.py:36-69: the model over `coordinates` (lats, lons), or over the uniform global axes of the metadata."""
    if coordinates is not None:
        lats, longs = coordinates
    else:
        lats = np.linspace(start=-90, stop=90, num=dataset_metadata.num_latitudes, endpoint=True)
        longs = np.linspace(start=0, stop=360, num=dataset_metadata.num_longitudes, endpoint=False)
    return WeatherPrediction(cordinates=(lats, longs), graph_config=experiment_config.graph,
                             pipeline_config=experiment_config.pipeline, data_config=experiment_config.data,
                             device=device, region_bounds=region_bounds, mesh_buffer=mesh_buffer, flat_grid=flat_grid)


def detect_region_bounds(coordinates):
    """src/main.py:150-165: axes that span less than 90 degrees both ways are a regional dataset, whose bounds
    (lat_min, lat_max, lon_min, lon_max) prune the mesh; None otherwise."""
    if coordinates is None:
        return None
    lats, lons = coordinates
    if float(lats.max() - lats.min()) < 90 and float(lons.max() - lons.min()) < 90:
        return float(lats.min()), float(lats.max()), float(lons.min()), float(lons.max())
    return None


def load_datasets(experiment_config: ExperimentConfig, data_root: str, device):
    """The dataset choice of src/main.py:81-124: (train, val, test, metadata)."""
    name = str(getattr(experiment_config.data.dataset_name, "value", experiment_config.data.dataset_name))
    data_dir = getattr(experiment_config, "data_dir", None)
    if data_dir or name in CHUNKED_DATASET_NAMES:
        if data_dir:
            data_path = data_dir
        elif name == "multires":
            data_path = os.path.join(data_root, name)
        else:  # v2 trains on the v1 series
            data_path = os.path.join(data_root, "global_512x256_19f_2010-2021_07deg")
        return load_chunked_datasets(data_path=data_path, obs_window=experiment_config.data.obs_window_used,
                                     pred_steps=max(experiment_config.max_ar_steps, 1),  # the AR targets
                                     n_features=experiment_config.data.num_features_used, device=device)
    return load_train_and_test_datasets(data_path=os.path.join(data_root, name), data_config=experiment_config.data,
                                        device=device)


def run_experiment(experiment_config: ExperimentConfig, results_save_dir: str, resume: bool = False,
                   pretrained_ckpt: str = None, *, data_root: str = os.path.join("data", "datasets"), device=None,
                   use_graph=None):
    """src/main.py:72-233.  Returns `train()`'s results dictionary."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("run_experiment needs a GPU (the HIP path has no CPU fallback)")
        device = "cuda:0"
    device = torch.device(device)
    print(f"Using device: {device}")
    set_random_seeds(seed=experiment_config.random_seed)

    train_dataset, val_dataset, test_dataset, dataset_metadata = load_datasets(experiment_config, data_root, device)
    bs = experiment_config.batch_size
    train_dataloader = DeviceLoader(train_dataset, batch_size=bs, shuffle=True)
    val_dataloader = DeviceLoader(val_dataset, batch_size=bs, shuffle=False)
    test_dataloader = DeviceLoader(test_dataset, batch_size=bs, shuffle=False)

    real_coords = getattr(dataset_metadata, "cordinates", None)
    flat_grid = getattr(dataset_metadata, "flat_grid", False)
    region_bounds = detect_region_bounds(real_coords)
    if region_bounds is not None:
        print(f"[region] regional dataset lat=[{region_bounds[0]:.1f},{region_bounds[1]:.1f}] "
              f"lon=[{region_bounds[2]:.1f},{region_bounds[3]:.1f}]: the mesh is pruned to it")
    model = load_model_from_experiment_config(experiment_config=experiment_config, device=device,
                                              dataset_metadata=dataset_metadata, coordinates=real_coords,
                                              region_bounds=region_bounds, flat_grid=flat_grid)
    model = model.to(device)

    pretrained = bool(pretrained_ckpt) and os.path.exists(pretrained_ckpt)
    if pretrained:
        print(f"\n>>> Loading pretrained weights: {pretrained_ckpt}")
        state = torch.load(pretrained_ckpt, map_location=device, weights_only=True)
        missing, unexpected = model.load_state_dict(state, strict=False)  # buffers of another grid are skipped
        if missing:
            print(f"  Missing keys ({len(missing)}): {missing[:5]}...")
        if unexpected:
            print(f"  Unexpected keys ({len(unexpected)}): {unexpected[:5]}...")

    # the reference groups the parameters whenever --pretrained is given, whether or not the file exists (:195)
    optimizer = build_optimizer(model, experiment_config, pretrained=bool(pretrained_ckpt))
    checkpoint_path = os.path.join(results_save_dir, FileNames.CHECKPOINT) if resume else None
    evaluator = Evaluator(model, use_graph=use_graph, **loss_masks(experiment_config, dataset_metadata, device))
    val_dataloader.buffers = evaluator.input_buffers  # full validation batches land in the captured graph's inputs
    return train(model=model, train_dataloader=train_dataloader, val_dataloader=val_dataloader,
                 test_dataloader=test_dataloader, optimiser=optimizer, num_epochs=experiment_config.num_epochs,
                 device=device, config=experiment_config, results_save_dir=results_save_dir,
                 dataset_metadata=dataset_metadata, print_losses=True, wandb_log=experiment_config.wandb_log,
                 resume_checkpoint=checkpoint_path, use_graph=use_graph, evaluator=evaluator)


def parse_args(argv):
    """The reference's argument handling (src/main.py:236-244): the experiment directory first, `--resume` and
    `--pretrained <path>` anywhere.  Returns (experiment_directory, resume, pretrained_ckpt) or exits with the usage."""
    argv = list(argv)
    if argv and argv[0] in ("-h", "--help"):
        print(USAGE)
        raise SystemExit(0)
    if not argv or argv[0].startswith("--"):
        print(USAGE, file=sys.stderr)
        raise SystemExit(2)
    pretrained_ckpt = None
    if "--pretrained" in argv:
        i = argv.index("--pretrained")
        if i + 1 >= len(argv):
            print(USAGE, file=sys.stderr)
            raise SystemExit(2)
        pretrained_ckpt = argv[i + 1]
    return argv[0], "--resume" in argv, pretrained_ckpt


def main(argv=None, **run_kwargs):
    """src/main.py:236-260.  `run_kwargs` (data_root, device, use_graph) go to `run_experiment`."""
    experiment_directory, resume, pretrained_ckpt = parse_args(sys.argv[1:] if argv is None else argv)
    results_save_dir = os.path.join(experiment_directory, RESULTS_FOLDER)
    os.makedirs(results_save_dir, exist_ok=True)
    experiment_config = ExperimentConfig(**load_from_json_file(os.path.join(experiment_directory,
                                                                            FileNames.EXPERIMENT_CONFIG)))
    return run_experiment(experiment_config=experiment_config, results_save_dir=results_save_dir, resume=resume,
                          pretrained_ckpt=pretrained_ckpt, **run_kwargs)


if __name__ == "__main__":
    main()
