"""Generate the fine-tuning fixture by RUNNING the reference's own `src/train.py::train` (src/train.py:311-524) on the
CPU, with the two-group optimiser of src/main.py:190-211, driving the stub of tests/helpers/finetune_stub.py.

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_finetune_golden.py

Output (data only - arrays and strings, no reference source text): tests/golden/finetune_vectors.npz
  init_<param>          the stub's initial parameters (every run starts from them)
  X_train, y_train, ...  the batches (finetune_stub.data())
  Per run r in (a, b, c), see finetune_stub.RUNS:
  r_train_losses, r_val_losses   per epoch, as train() returns them (and writes to results.json)
  r_val_acc, r_ar, r_patience    per epoch: the validation ACC, the AR level and the patience counter after the epoch
  r_init_val                     (loss, ACC, RMSE) of the initial validation (runs starting at epoch 0)
  r_stop_epoch                   the epoch (1-based) early stopping ended the run at, else 0
  r_log                          training_log.txt without its timestamps
  r_final_<param>, r_best_<param>  parameters at the end and those of best_model.pth
  r_opt_<k>_step / _exp_avg / _exp_avg_sq   final torch.optim.Adam state of state index k (absent: never stepped)
  r_opt_lr, r_opt_params<g>      lr of every parameter group, state indices of group g
  Run c is 3 epochs then a resume to 5 from checkpoint.pth; c1_* holds the same for the first part and
  c1_ckpt_* the checkpoint it wrote (epoch, ar_steps, best_val_loss, patience_counter, model and optimiser state).
"""
import contextlib
import io
import os
import re
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_golden  # noqa: E402  (where the reference checkout lives, placeholder modules)
import finetune_stub as S  # noqa: E402

REF = make_golden.REF


def optimiser_of(model, cfg):
    """The optimiser src/main.py:190-211 builds for a pretrained model (restated: the reference builds it inline)."""
    proc = list(model.processor.parameters())
    ids = {id(p) for p in proc}
    other = [p for p in model.parameters() if id(p) not in ids]
    for p in proc:
        p.requires_grad = False
    return torch.optim.Adam([{"params": other, "lr": cfg.learning_rate},
                             {"params": proc, "lr": cfg.learning_rate * cfg.finetune_processor_lr_factor}])


def strip_log(path):
    """training_log.txt without timestamps (the trailing HH:MM:SS of the table rows, the ISO stamps of the banners)."""
    out = []
    for line in open(path).read().splitlines():
        line = re.sub(r"\s*\d{2}:\d{2}:\d{2}$", "", line)
        line = re.sub(r": \d{4}-\d{2}-\d{2}T[\d:.]+ ===$", " ===", line)
        out.append(line)
    return out


def opt_state(prefix, sd, out):
    for k, st in sd["state"].items():
        out[f"{prefix}_opt_{k}_step"] = np.float64(float(st["step"]))
        out[f"{prefix}_opt_{k}_exp_avg"] = st["exp_avg"].numpy().copy()
        out[f"{prefix}_opt_{k}_exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
    out[f"{prefix}_opt_lr"] = np.array([g["lr"] for g in sd["param_groups"]], dtype=np.float64)
    for gi, g in enumerate(sd["param_groups"]):
        out[f"{prefix}_opt_params{gi}"] = np.array(g["params"], dtype=np.int64)


def run_part(prefix, cfg, epochs, out, train_b, val_b, resume=None, workdir=None):
    """One call of the reference's train(); records what the module's train_epoch / test saw and returned."""
    import src.train as RT

    model = S.FinetuneStub()
    if resume is None:
        model.load_state_dict({k: torch.tensor(out[f"init_{k}"]) for k, _ in model.named_parameters()})
    opt = optimiser_of(model, cfg)
    seen = {"ar": [], "val": []}
    orig_epoch, orig_test = RT.train_epoch, RT.test

    def rec_epoch(*a, **k):
        seen["ar"].append(k["current_ar_steps"])
        return orig_epoch(*a, **k)

    def rec_test(*a, **k):
        r = orig_test(*a, **k)
        seen["val"].append(r)
        return r

    RT.train_epoch, RT.test = rec_epoch, rec_test
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            res = RT.train(model, train_b, val_b, None, opt, epochs, "cpu", cfg, workdir,
                           dataset_metadata=S.metadata(), print_losses=True, wandb_log=False,
                           resume_checkpoint=resume)
    finally:
        RT.train_epoch, RT.test = orig_epoch, orig_test
    log = strip_log(os.path.join(workdir, "training_log.txt"))
    rows = [line for line in log if re.match(r"^\s+\d+\s+\d+\s", line)]
    vals = seen["val"][1:] if resume is None else seen["val"]
    if resume is None:
        out[f"{prefix}_init_val"] = np.array(seen["val"][0], dtype=np.float64)
    out[f"{prefix}_train_losses"] = np.array(res["train_losses"], dtype=np.float64)
    out[f"{prefix}_val_losses"] = np.array(res["val_losses"], dtype=np.float64)
    out[f"{prefix}_val_acc"] = np.array([v[1] for v in vals], dtype=np.float64)
    out[f"{prefix}_ar"] = np.array(seen["ar"], dtype=np.int64)
    out[f"{prefix}_patience"] = np.array([int(r.split()[6]) for r in rows], dtype=np.int64)
    stop = [line for line in log if "Early stopping" in line]
    out[f"{prefix}_stop_epoch"] = np.int64(int(stop[0].split()[-1]) if stop else 0)
    out[f"{prefix}_log"] = np.array(log)
    for k, p in model.named_parameters():
        out[f"{prefix}_final_{k}"] = p.detach().numpy().copy()
    best = torch.load(os.path.join(workdir, "best_model.pth"), weights_only=True)
    for k, _ in model.named_parameters():
        out[f"{prefix}_best_{k}"] = best[k].numpy().copy()
    opt_state(prefix, opt.state_dict(), out)
    ckpt = torch.load(os.path.join(workdir, "checkpoint.pth"), weights_only=True)
    return ckpt


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    make_golden._placeholders()
    sys.path.insert(0, REF)
    import src.train  # noqa: F401

    out = {}
    m0 = S.FinetuneStub()
    for k, p in m0.named_parameters():
        out[f"init_{k}"] = p.detach().numpy().copy()
    train_b, val_b = S.data()
    out["X_train"] = torch.stack([x for x, _ in train_b]).numpy()
    out["y_train"] = torch.stack([y for _, y in train_b]).numpy()
    out["X_val"] = torch.stack([x for x, _ in val_b]).numpy()
    out["y_val"] = torch.stack([y for _, y in val_b]).numpy()
    for r, (over, epochs, split) in S.RUNS.items():
        cfg = S.config(**over)
        with tempfile.TemporaryDirectory() as d:
            if split is None:
                run_part(r, cfg, epochs, out, train_b, val_b, workdir=d)
                continue
            ckpt = run_part(f"{r}1", cfg, split, out, train_b, val_b, workdir=d)
            for k in ("epoch", "ar_steps", "best_val_loss", "patience_counter"):
                out[f"{r}1_ckpt_{k}"] = np.float64(ckpt[k])
            for k, v in ckpt["model_state_dict"].items():
                out[f"{r}1_ckpt_model_{k}"] = v.numpy().copy()
            opt_state(f"{r}1_ckpt", ckpt["optimizer_state_dict"], out)
            # resume: a fresh model and the optimiser of src/main.py (processor frozen again), as main(resume=True)
            run_part(r, cfg, epochs, out, train_b, val_b, resume=os.path.join(d, "checkpoint.pth"), workdir=d)
            for k in ("val_acc", "ar"):  # the whole run's epochs (the log and the loss lists already span both parts)
                out[f"{r}_{k}"] = np.concatenate([out[f"{r}1_{k}"], out[f"{r}_{k}"]])
            out[f"{r}_init_val"] = out[f"{r}1_init_val"]
    np.savez_compressed(os.path.join(HERE, "finetune_vectors.npz"), **out)
    print("wrote", os.path.join(HERE, "finetune_vectors.npz"), f"({os.path.getsize(os.path.join(HERE, 'finetune_vectors.npz'))} bytes)")


if __name__ == "__main__":
    main()
