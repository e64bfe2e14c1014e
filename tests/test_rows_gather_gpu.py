"""svla_rows_gather (csrc/rows.hip) through ops.rows_gather, bit for bit against torch indexing: dst[r] = idx[r] >= 0 ? src[idx[r]] : 0 over rows of 16 bytes (one
vector), 1 KiB (a bf16 row of the 512-wide transformer) and 258 048 bytes (a 224 x 384 x 3 camera frame); 9 destination rows out of 5 source rows with -1 entries
(zero rows) and a repeated row; dense and padded strides on either side, the bytes between the rows untouched; a row count beyond one pass of the largest grid; an
index past the source (zeros, nothing read); svla_fusion_text_bwd_seg against a torch sum; and the refusals, which launch nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDX = [3, -1, 0, 4, -1, 2, 2, 1, -1]          # 9 rows out of 5; rows 1, 4 and 8 are zero rows


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _want(src, idx, row_bytes):
    """src uint8 [src_rows, stride] -> uint8 [rows, row_bytes] by torch indexing"""
    idx = torch.as_tensor(idx, device=src.device, dtype=torch.int64)
    ok = (idx >= 0) & (idx < src.shape[0])
    rows = src[idx.clamp(0, src.shape[0] - 1), :row_bytes]
    return torch.where(ok[:, None], rows, torch.zeros_like(rows))


@pytest.mark.parametrize("row_bytes", [16, 1024, 258048])
@pytest.mark.parametrize("pad_dst,pad_src", [(0, 0), (48, 16), (16, 4096)])
def test_gather_is_bitwise_torch_indexing(row_bytes, pad_dst, pad_src):
    _need_gpu()
    from safevla_amd import ops

    g = torch.Generator(device=DEV).manual_seed(row_bytes + pad_dst)
    ss, ds = row_bytes + pad_src, row_bytes + pad_dst
    src = torch.randint(0, 256, (5, ss), device=DEV, dtype=torch.uint8, generator=g)
    dst = torch.full((len(IDX), ds), 0xA5, device=DEV, dtype=torch.uint8)
    idx = torch.tensor(IDX, device=DEV, dtype=torch.int32)
    ops.rows_gather(dst, ds, src, ss, idx, len(IDX), row_bytes, 5)
    torch.cuda.synchronize()
    assert torch.equal(dst[:, :row_bytes], _want(src, IDX, row_bytes))
    assert (dst[:, row_bytes:] == 0xA5).all()          # the bytes between the rows are not written
    assert (dst[[1, 4, 8], :row_bytes] == 0).all()


def test_gather_typed_rows_many_rows_and_an_index_past_the_source():
    """bf16 rows of the transformer ([rows, 512] out of a [R, S, 512] token buffer: source stride S * 1 KiB), more vectors than one pass of 2048 workgroups x 256
    lanes x 4 covers (40 000 rows x 64 vectors), and indices >= src_rows, which store zeros like -1 does"""
    _need_gpu()
    from safevla_amd import ops

    g = torch.Generator(device=DEV).manual_seed(1)
    R, S, D, rows = 37, 3, 512, 40000
    src = torch.randn(R, S, D, device=DEV, generator=g).bfloat16()
    idx = torch.randint(-1, R + 2, (rows,), device=DEV, generator=g).to(torch.int32)
    dst = torch.empty(rows, D, device=DEV, dtype=torch.bfloat16)
    ops.rows_gather(dst, D * 2, src, S * D * 2, idx, rows, D * 2, R)
    torch.cuda.synchronize()
    ok = (idx >= 0) & (idx < R)
    want = torch.where(ok[:, None], src[idx.long().clamp(0, R - 1), 0], torch.zeros((), device=DEV, dtype=torch.bfloat16))
    assert ok.sum() < rows and torch.equal(dst.view(torch.int16), want.view(torch.int16))


def test_inverse_table_round_trip():
    """compact -> padded through the map, padded -> compact through its inverse: the compact rows come back bit for bit (the map is injective), into a strided destination"""
    _need_gpu()
    from safevla_amd import ops

    g = torch.Generator(device=DEV).manual_seed(2)
    fwd = torch.tensor([0, 8, 13, 1, 9, -1, 2, 10, -1, 3, 11, -1, 4, 12, -1, 5, -1, -1, 6, -1, -1, 7, -1, -1], device=DEV, dtype=torch.int32)      # B = 3, T = 8, lengths 8, 5, 1
    inv = torch.empty(14, device=DEV, dtype=torch.int32)
    inv[fwd[fwd >= 0].long()] = torch.nonzero(fwd >= 0).reshape(-1).to(torch.int32)
    x = torch.randn(14, 512, device=DEV, generator=g).bfloat16()
    padded = torch.empty(24, 512, device=DEV, dtype=torch.bfloat16)
    ops.rows_gather(padded, 1024, x, 1024, fwd, 24, 1024, 14)
    back = torch.zeros(14, 5, 512, device=DEV, dtype=torch.bfloat16)
    ops.rows_gather(back, 5 * 1024, padded, 1024, inv, 14, 1024, 24)
    torch.cuda.synchronize()
    assert torch.equal(back[:, 0].view(torch.int16), x.view(torch.int16)) and (back[:, 1:] == 0).all()
    assert (padded[fwd < 0] == 0).all()


def test_refusals_launch_nothing():
    _need_gpu()
    from safevla_amd import ops
    from safevla_amd._lib import SvlaError, lib

    L = lib()
    src = torch.zeros(5, 1024, device=DEV, dtype=torch.uint8)
    dst = torch.full((9, 1024), 7, device=DEV, dtype=torch.uint8)
    idx = torch.tensor(IDX, device=DEV, dtype=torch.int32)
    good = dict(dst=dst, dst_stride=1024, src=src, src_stride=1024, idx=idx, rows=9, row_bytes=1024, src_rows=5)
    # refused by the Python binding: no C-ABI call at all
    for over in (dict(rows=0), dict(rows=-1), dict(row_bytes=1000), dict(row_bytes=8), dict(dst_stride=1008), dict(src_stride=512), dict(rows=10), dict(src_rows=6),
                 dict(idx=idx[:8]), dict(idx=idx.cpu()), dict(idx=idx.long())):
        calls = []
        assert L.recorder is None
        L.recorder = calls
        try:
            with pytest.raises((ValueError, TypeError)):
                ops.rows_gather(**{**good, **over})
        finally:
            L.recorder = None
        assert calls == [], over
    # refused by the entry point itself (SVLA_EINVAL before any launch): the issue's four, straight through the C ABI
    s = ops._stream()
    for args in ((dst.data_ptr(), 1024, src.data_ptr(), 1024, idx.data_ptr(), 0, 1024, 5, s), (dst.data_ptr(), 1024, src.data_ptr(), 1024, idx.data_ptr(), 9, 1000, 5, s),
                 (dst.data_ptr(), 1008, src.data_ptr(), 1024, idx.data_ptr(), 9, 1024, 5, s), (dst.data_ptr(), 1024, src.data_ptr(), 1024, None, 9, 1024, 5, s)):
        with pytest.raises(SvlaError, match="invalid argument"):
            L.call("svla_rows_gather", *args)
    torch.cuda.synchronize()
    assert (dst == 7).all()


def test_fusion_text_bwd_seg_against_torch():
    """dtext[u, j] = the sum of dx0[r, text_off + j] over the goal's compact rows; an empty segment gives zeros; fp32 sums of bf16 rows in row order -- the torch sum
    of the same bf16 values in fp64 differs by fp32 rounding of at most 8 terms: 8 * 2^-24 relative to the sum of magnitudes"""
    _need_gpu()
    from safevla_amd import ops

    g = torch.Generator(device=DEV).manual_seed(3)
    U, S, L, off, D = 4, 9, 3, 5, 768
    seg = [0, 8, 8, 13, 14]                                  # goal 1 has no rows
    dx0 = torch.randn(14, S, D, device=DEV, generator=g).bfloat16()
    dtext = torch.full((U, L, D), float("nan"), device=DEV)
    ops.fusion_text_bwd_seg(dx0, torch.tensor(seg, device=DEV, dtype=torch.int32), U, S, L, off, dtext)
    torch.cuda.synchronize()
    for u in range(U):
        rows = dx0[seg[u]:seg[u + 1], off:off + L].double()
        want, mag = rows.sum(0), rows.abs().sum(0)
        assert ((dtext[u].double() - want).abs() <= 8 * 2.0 ** -24 * mag).all(), u
    assert (dtext[1] == 0).all()
