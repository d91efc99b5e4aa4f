"""Contract of `gcl_tensor_batch_pack` (csrc/dataset.hip) as include/gcl.h states it: plain copies, so every comparison
is `torch.equal` with torch's own indexing of the stored tensor."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (N, G, W, F, Wu, Fu): a partial selection, the smallest tensor, rows of 66 floats over more than one block
CASES = [(5, 24, 3, 5, 2, 3), (4, 7, 1, 1, 1, 1), (6, 130, 5, 33, 2, 33)]


def _stores(N, G, W, F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, G, W, F, generator=g).to(DEV), torch.randn(N, G, max(W - 1, 1), F, generator=g).to(DEV)


def _want(src, idx, Wu, Fu):
    W = src.shape[2]
    return src[idx][:, :, W - Wu:, :Fu].reshape(len(idx), src.shape[1], Wu * Fu)


def _indices(N):
    return [list(range(N)), list(range(N - 1, -1, -1)), [N - 1, 0, 0, N // 2, 0, N - 1, N // 2]]


@pytest.mark.parametrize("N,G,W,F,Wu,Fu", CASES)
def test_pack_equals_torch_indexing(N, G, W, F, Wu, Fu, lib_built):
    from graphcast_lite_amd import hip

    X4, Y4 = _stores(N, G, W, F, N + G)
    Wyu = min(Wu, Y4.shape[2])
    for idx in _indices(N):  # ascending, descending, repeated and unordered
        t = torch.tensor(idx, dtype=torch.int64, device=DEV)
        X, Y = hip.tensor_batch_pack(X4, Y4, t, Wu, Wyu, Fu)
        assert X.shape == (len(idx), G, Wu * Fu) and Y.shape == (len(idx), G, Wyu * Fu)
        assert torch.equal(X, _want(X4, t, Wu, Fu)) and torch.equal(Y, _want(Y4, t, Wyu, Fu))
        X1, none = hip.tensor_batch_pack(X4, None, t, Wu, 0, Fu)  # X alone
        assert none is None and torch.equal(X1, X)


@pytest.mark.parametrize("N,G,W,F,Wu,Fu", CASES)
def test_pack_into_padded_offset_buffers(N, G, W, F, Wu, Fu, lib_built):
    from graphcast_lite_amd import hip

    X4, Y4 = _stores(N, G, W, F, 3 * N + G)
    Wyu = min(Wu, Y4.shape[2])
    idx = torch.tensor(_indices(N)[2], dtype=torch.int64, device=DEV)
    B = idx.numel()
    wideX = torch.full((B + 2, G + 3, Wu * Fu + 5), -7.0, device=DEV)
    wideY = torch.full((B + 1, G + 1, Wyu * Fu + 2), -7.0, device=DEV)
    outX, outY = wideX[1:B + 1, 2:G + 2, 3:3 + Wu * Fu], wideY[1:, :G, 1:1 + Wyu * Fu]
    X, Y = hip.tensor_batch_pack(X4, Y4, idx, Wu, Wyu, Fu, out=(outX, outY))
    assert X.data_ptr() == outX.data_ptr() and Y.data_ptr() == outY.data_ptr()
    assert torch.equal(outX, _want(X4, idx, Wu, Fu)) and torch.equal(outY, _want(Y4, idx, Wyu, Fu))
    for wide, out in ((wideX, outX), (wideY, outY)):
        rest = wide.clone()
        rest.as_strided(out.shape, out.stride(), out.storage_offset() - wide.storage_offset()).fill_(-7.0)
        assert bool((rest == -7.0).all())


@pytest.mark.parametrize("bad", [-1, 5, 1 << 40])
def test_out_of_range_index_gives_nan_rows_for_that_sample_only(bad, lib_built):
    from graphcast_lite_amd import hip

    N, G, W, F, Wu, Fu = CASES[0]
    X4, Y4 = _stores(N, G, W, F, 9)
    idx = torch.tensor([3, bad, 0], dtype=torch.int64, device=DEV)
    X, Y = hip.tensor_batch_pack(X4, Y4, idx, Wu, 1, Fu)
    ok = torch.tensor([3, 0], dtype=torch.int64, device=DEV)
    for got, src, wu in ((X, X4, Wu), (Y, Y4, 1)):
        assert bool(torch.isnan(got[1]).all())
        assert torch.equal(got[[0, 2]], _want(src, ok, wu, Fu))


def test_wrapper_rejects_mismatched_buffers(lib_built):
    from graphcast_lite_amd import hip

    X4, Y4 = _stores(5, 24, 3, 5, 1)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        hip.tensor_batch_pack(X4, Y4, idx, 2, 1, 3, out=(torch.empty(2, 24, 7, device=DEV), torch.empty(2, 24, 3, device=DEV)))
    with pytest.raises(ValueError):
        hip.tensor_batch_pack(X4, Y4[:, :23], idx, 2, 1, 3)
    with pytest.raises(RuntimeError, match="4 of 3 stored steps"):
        hip.tensor_batch_pack(X4, Y4, idx, 4, 1, 3)
