"""A stand-in for the downscaler's network in the tests: a seeded 1x1 channel mix out[b, o] = sum_i W[o, i] X[b, i] in
plain torch ops.  Test-only."""
import torch


class ChannelMix(torch.nn.Module):
    def __init__(self, c_in: int, c_out: int, seed: int = 7, scale: float = 0.1):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        w = scale * torch.randn(c_out, c_in, generator=g, dtype=torch.float64)
        self.weight = torch.nn.Parameter(w.to(torch.float32))

    def forward(self, X):
        return torch.einsum("oi,bihw->bohw", self.weight, X)
