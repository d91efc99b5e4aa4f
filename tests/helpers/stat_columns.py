"""Columns for the column-statistics contract tests (test_scoring_kernels, test_map_kernels): one pool of normal
deviates, drawn once, from which every case cuts its rows, and the three kinds of column the shifted one-pass sums of
the kernels are built for.  Everything here runs on the device its inputs are on."""
import torch

# 64-row chunks; 512 chunks of 64, then 505 of 65 (8 row lanes x 4); 197: a last chunk of 5 rows, fewer than the row
# lanes; 32835: 506 chunks of 65, the last of 10 rows (appended, so that the earlier cases keep their seeds)
NS = [1, 7, 8, 9, 63, 64, 65, 96, 129, 32768, 32769, 197, 32835]
KS = [1, 19, 31, 32, 33]  # 32-column tiles
GMAX, WMAX = max(NS) + 5, KS[-1] + 3


def deviates(n_rows, seed=20240):
    """Standard normal deviates [5, 3, n_rows, WMAX]: [0] the truth's, [1 + q] those of prediction q."""
    return torch.randn(5, 3, n_rows, WMAX, generator=torch.Generator().manual_seed(seed))


def columns(z, first):
    """Truth [B, G, WMAX] and four predictions from deviates z [5, B, G, WMAX].  Column k is ordinary (k % 3 == 0),
    has its mean at 1e4 sigma (k % 3 == 1) or is constant in the truth (k % 3 == 2; odd predictions are constant
    there too).  Row `first`, the first scored one, gets the deviate 0.5, so that it lies within 4 sigma of every
    column's mean whatever the draw (the tests assert that it does)."""
    z = z.clone()
    z[:, :, first, :] = 0.5
    kind = torch.arange(z.shape[-1], device=z.device) % 3
    t = torch.where(kind == 0, 0.3 + 1.5 * z[0], torch.where(kind == 1, 1e4 + z[0], torch.full_like(z[0], 2.5)))
    preds = []
    for q in range(4):
        p = t + 0.5 * (q + 1) * z[1 + q]
        preds.append(torch.where(kind == 2, torch.full_like(p, 1.25), p) if q % 2 else p)
    return t, preds


def row_list(n, g):
    """n scored rows of a field of n + 5: unsorted, none below row 2, the last a duplicate of the first (n > 1)."""
    r = 2 + torch.randperm(n + 3, generator=g)[:n]
    if n > 1:
        r[n - 1] = r[0]
    return r


def first_row_within_4_sigma(X):
    """The condition the one-pass bounds rest on, for X [B, n, K] float64: row 0 within 4 sigma of the column mean."""
    std = X.std(1, unbiased=False) if X.shape[1] > 1 else torch.zeros_like(X[:, 0])
    # |n x_0 - sum x| <= 4 n std, the condition times n: the device's mean (and its division by a scalar) multiplies by a
    # rounded 1 / n, which at n = 197 puts the mean of a constant column (std exactly 0) one ulp off its value, while
    # n x_0 and the sum of a constant column of float32 values are exact
    n = X.shape[1]
    return bool(((n * X[:, 0] - X.sum(1)).abs() <= 4 * n * std).all())
