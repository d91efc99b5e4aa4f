"""Child process of tests/test_value_contract.py::test_valu_kernels_*: GCL_LINEAR_IMPL is read once per process, so the
plain-VALU dense kernels run in a process of their own.  argv: repository root, file of jobs (a list of dicts with "op" =
"fwd" | "dx", the operands on the CPU and "act"), file for the results (a list of outputs on the CPU, and the names of the
kernels launched)."""
import os
import sys

import torch

root, jobs_path, out_path = sys.argv[1:4]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests", "helpers"))
from layouts import DEV, launched  # noqa: E402

from graphcast_lite_amd import hip  # noqa: E402


def run(job):
    a = torch.tensor([0.25], device=DEV) if job["act"] == 1 else None
    if job["op"] == "fwd":
        return hip.dense_fwd(job["x"].to(DEV), job["W"].to(DEV), job["b"].to(DEV), job["act"], a).cpu()
    ds = torch.full((1,), 0.125, device=DEV)
    dx = hip.dense_bwd_dx(job["dy"].to(DEV), job["W"].to(DEV), job["z"].to(DEV) if job["act"] else None, job["act"], a,
                          ds if job["act"] == 1 else None)
    return [dx.cpu(), ds.cpu()]


outs, names = launched(lambda: [run(job) for job in torch.load(jobs_path)])
torch.save({"outs": outs, "names": names}, out_path)
