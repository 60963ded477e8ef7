"""The small kernels of csrc/runtime.hip (and `split_f16` of csrc/gemm_f32.hip) in every form a step can reach them in:
vector body, scalar tail and the unaligned all-tail path of `convert`; `copy2d` and `gather_rows` with pitches, in both
dtypes, past their grid-stride block caps (4096 / 8192 / 8192 / 2048 blocks of 256 threads); the no-zeroing, several-producer
contract of `absmax_fold`; `zero_words`.  Every reference is plain torch on the host and every comparison is bit for bit;
whatever lies around a destination carries a sentinel that must survive.
"""
import pytest
import torch

from aurora_amd.engine import lib as L
from tests.perceiver_reference import unsplit

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF, NAN = float("inf"), float("nan")


def _f32(bits):
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


# fp32 -> bf16 edge values: +-0, +-inf, NaN, subnormals, ties to even in both directions (low half 0x8000 under an even /
# an odd kept bit), ties just missed, the largest finite fp32 (rounds to inf) and 0x7f7f8000, a tie that rounds to bf16 inf
EDGES_F32 = _f32([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x00000001, 0x807fffff, 0x00008000, 0x00018000,
                  0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x7f7fffff, 0xff7fffff, 0x7f7f8000])
# bf16 -> fp32 is exact: +-0, +-inf, NaN, bf16 subnormals, the largest finite value
EDGES_BF16 = torch.tensor([0x0000, -0x8000, 0x7f80, -0x80, 0x7fc0, 0x0001, -0x7fff, 0x007f, 0x7f7f, -0x81],
                          dtype=torch.int16).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(out, ref):
    """Bit for bit, NaN compared as `is NaN`."""
    nan = torch.isnan(ref)
    return torch.equal(torch.isnan(out), nan) and torch.equal(_bits(out)[~nan], _bits(ref)[~nan])


def _convert_input(n, dtype):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(dtype)
    e = EDGES_F32 if dtype == torch.float32 else EDGES_BF16
    k = min(n, e.numel())
    x[:k] = e[:k]                        # the vector body (when there is one)
    x[n - k:] = e[e.numel() - k:]        # ... and the end: the last n % 8 elements are the scalar tail
    t = n % 8
    if 0 < t < n:
        x[n - t:] = e[torch.arange(t) % 5 + 9] if dtype == torch.float32 else e[torch.arange(t) % e.numel()]   # ties in the tail
    return x


CONVERT_N = [1, 7, 8, 9, 255, 2049, 8 * 256 * 4096 + 8 * 300 + 5]   # the last: past 4096 blocks (the loop wraps) and a tail of 5


@pytest.mark.parametrize("offsets", [(0, 0), (1, 0), (0, 1)], ids=["aligned", "src+1", "dst+1"])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16], ids=["f32_to_bf16", "bf16_to_f32"])
@pytest.mark.parametrize("n", CONVERT_N)
def test_convert_body_tail_and_unaligned_path(n, src_dtype, offsets):
    """Aligned operands take 8 elements per thread and `convert_tail_kernel` for the last n % 8; an operand that is not
    16-byte aligned sends every element through the tail kernel.  fp32 -> bf16 rounds to nearest even."""
    dst_dtype = torch.bfloat16 if src_dtype == torch.float32 else torch.float32
    so, do = offsets
    x = _convert_input(n, src_dtype)
    src = torch.zeros(n + 16, dtype=src_dtype, device=DEV)
    src[so:so + n] = x.to(DEV)
    buf = torch.full((n + 32,), -7.0, dtype=dst_dtype, device=DEV)
    dst = buf[8 + do:8 + do + n]
    assert (src.data_ptr() % 16 == 0) and (buf.data_ptr() % 16 == 0)
    L.convert(src[so:so + n], dst)
    torch.cuda.synchronize()
    out = buf.cpu()
    assert _same(out[8 + do:8 + do + n], x.to(dst_dtype))
    assert bool((out[:8 + do] == -7.0).all()) and bool((out[8 + do + n:] == -7.0).all())   # nothing around it is written


def test_convert_edge_values_one_by_one():
    """Every edge value alone (n = 1: tail kernel) and as a whole vector of 8 (body), so that none hides behind another."""
    for e, dd in ((EDGES_F32, torch.bfloat16), (EDGES_BF16, torch.float32)):
        x = e.repeat_interleave(8)
        out = L.convert(x.to(DEV), torch.empty(x.numel(), dtype=dd, device=DEV)).cpu()
        assert _same(out, x.to(dd))
        for i in range(e.numel()):
            one = L.convert(e[i:i + 1].to(DEV), torch.empty(1, dtype=dd, device=DEV)).cpu()
            assert _same(one, e[i:i + 1].to(dd)), i
    assert EDGES_F32[-1].bfloat16().item() == INF and EDGES_F32[8].bfloat16().item() != EDGES_F32[7].bfloat16().item()


def _matrix(rows, cols, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,col_bytes", [(1, 16), (3, 16), (1000, 16), (1, 48), (3, 48), (1000, 48), (4100, 8192)])
def test_copy2d_pitched_blocks(rows, col_bytes, dtype):
    """A column block of a pitched source into a column block of a wider destination.  (4100, 8192 bytes): 2,099,200 pieces,
    past 8192 blocks of 256."""
    es = 2 if dtype == torch.bfloat16 else 4
    cols, pad = col_bytes // es, 16 // es
    src_full = _matrix(rows, cols + 2 * pad, dtype, rows + col_bytes)
    dst_full = torch.full((rows, cols + 3 * pad), -7.0, dtype=dtype)
    s, d = src_full.to(DEV), dst_full.to(DEV)
    L.copy2d(s[:, pad:pad + cols], d[:, 2 * pad:2 * pad + cols])
    torch.cuda.synchronize()
    want = dst_full.clone()
    want[:, 2 * pad:2 * pad + cols] = src_full[:, pad:pad + cols]
    assert torch.equal(_bits(d.cpu()), _bits(want))
    assert torch.equal(s.cpu(), src_full)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_copy2d_refuses_rows_that_are_not_16_byte_pieces(dtype):
    es = 2 if dtype == torch.bfloat16 else 4
    e16 = 16 // es
    msg = "copy2d: rows must be 16-byte multiples and aligned"
    src = torch.ones((4, 4 * e16), dtype=dtype, device=DEV)
    dst = torch.full((4, 4 * e16), -7.0, dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match=msg):
        L.copy2d(src, dst, cols=e16 - 1)                                             # cols * es % 16 != 0
    odd = torch.ones((4, 4 * e16 + 1), dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match=msg):
        L.copy2d(odd[:, :e16], dst[:, :e16])                                         # source pitch
    odd_d = torch.full((4, 4 * e16 + 1), -7.0, dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match=msg):
        L.copy2d(src[:, :e16], odd_d[:, :e16])                                       # destination pitch
    with pytest.raises(ValueError, match=msg):
        L.copy2d(src[:, 1:1 + e16], dst[:, :e16])                                    # misaligned source pointer
    with pytest.raises(ValueError, match=msg):
        L.copy2d(src[:, :e16], dst[:, 1:1 + e16])                                    # misaligned destination pointer
    code = L.load().aurora_hip_copy2d(src.data_ptr(), 4 * e16, dst.data_ptr() + es, 4 * e16, 4, e16, L.dtype_code(dtype), None)
    assert code == -1 and msg.encode() in L.load().aurora_hip_last_error()
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all()) and bool((odd_d == -7.0).all())                # nothing was written


def _gather_idx(n_rows, n_src):
    """Repeats, the first row, the last row and a descending run."""
    if n_rows == 1:
        return torch.tensor([n_src - 1], dtype=torch.int32)
    if n_rows == 5:
        return torch.tensor([n_src - 1, 3, 2, 2, 0], dtype=torch.int32)
    i = torch.arange(n_rows, dtype=torch.int64)
    idx = (n_src - 1 - i) % n_src                  # descending runs from the last row to the first
    idx[1::7] = idx[0::7][:idx[1::7].numel()]      # repeats
    return idx.to(torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("row_bytes,n_rows", [(16, 1), (16, 5), (16, 70000), (48, 1), (48, 5), (48, 70000),
                                              (2048, 1), (2048, 5), (2048, 16500)])   # 16500 x 128 pieces: past 8192 blocks
def test_gather_rows_pitched(row_bytes, n_rows, dtype):
    es = 2 if dtype == torch.bfloat16 else 4
    w, pad, n_src = row_bytes // es, 16 // es, 611
    src_full = _matrix(n_src, w + pad, dtype, row_bytes + n_rows)
    dst_full = torch.full((n_rows, w + 2 * pad), -7.0, dtype=dtype)
    idx = _gather_idx(n_rows, n_src)
    assert int(idx.min()) == 0 or n_rows == 1
    assert int(idx.max()) == n_src - 1
    s, d = src_full.to(DEV), dst_full.to(DEV)
    L.gather_rows(s[:, :w], idx.to(DEV), d[:, :w])
    torch.cuda.synchronize()
    want = dst_full.clone()
    want[:, :w] = src_full[idx.long(), :w]
    assert torch.equal(_bits(d.cpu()), _bits(want))     # (the gap bytes of every destination row included)
    assert torch.equal(s.cpu(), src_full)


ABSMAX_N = [1, 2, 3, 4, 5, 1023, 2048 * 256 * 4 + 3]   # the last: past 2048 blocks, and a tail of 3


def _fold(x, word):
    L._check(L.load().aurora_hip_absmax_fold(x.data_ptr(), x.numel(), word.data_ptr(), L._stream()))


@pytest.mark.parametrize("n", ABSMAX_N)
def test_absmax_finds_the_maximum_wherever_it_is(n):
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g)
    for pos in sorted({0, n - 1, n - n % 4 if n % 4 else n - 1, n // 2}):   # first, last, first tail element, middle
        for v in (-77.25, 77.25):
            x = base.clone()
            x[pos] = v
            out = L.absmax(x.to(DEV))
            assert out.item() == 77.25, (pos, v)
    x = base.clone()
    x[n - 1] = NAN
    want = float(base[:n - 1].abs().max()) if n > 1 else 0.0
    assert L.absmax(x.to(DEV)).item() == want          # NaN is ignored (alone: the word stays 0)
    x[0] = -INF
    assert L.absmax(x.to(DEV)).item() == INF
    assert L.absmax(torch.full((n,), -0.0, device=DEV)).view(torch.int32).item() == 0   # |-0| is +0


@pytest.mark.parametrize("n", ABSMAX_N)
def test_absmax_fold_only_ever_raises_the_word(n):
    """`absmax_fold` does not clear its word: several producers fold into one, in any order, and a word that is already larger
    stays.  Its neighbours are never touched."""
    g = torch.Generator().manual_seed(n + 1)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    ma, mb = float(a.abs().max()), float(b.abs().max())
    a_d, b_d = a.to(DEV), b.to(DEV)
    words = torch.tensor([-5.0, 1000.0, -5.0], device=DEV)
    _fold(a_d, words[1:])
    assert words.tolist() == [-5.0, 1000.0, -5.0]                      # never lowered
    for first, second in ((a_d, b_d), (b_d, a_d)):
        words = torch.tensor([-5.0, 0.0, -5.0], device=DEV)
        _fold(first, words[1:])
        _fold(second, words[1:])
        assert words.tolist() == [-5.0, max(ma, mb), -5.0]
    words = torch.tensor([-5.0, 0.25, -5.0], device=DEV)
    _fold(torch.full((n,), NAN, device=DEV), words[1:])
    _fold(torch.full((n,), -0.0, device=DEV), words[1:])
    assert words.tolist() == [-5.0, 0.25, -5.0]                        # NaN and -0.0 fold nothing in
    x = a.clone()
    x[n - 1] = -INF
    _fold(x.to(DEV), words[1:])
    assert words.tolist() == [-5.0, INF, -5.0]
    _fold(b_d, words[1:])
    assert words[1].item() == INF


def test_absmax_refuses_a_misaligned_array():
    x = torch.ones(64, device=DEV)
    out = torch.full((1,), -5.0, device=DEV)
    with pytest.raises(ValueError, match="absmax: bad arguments"):
        _fold(x[1:], out)
    assert out.item() == -5.0
    with pytest.raises(ValueError, match="absmax: bad arguments"):
        L.absmax(x[2:], out)


@pytest.mark.parametrize("n", [1, 4, 64])
def test_zero_words_clears_exactly_n(n):
    w = torch.arange(1, 67, dtype=torch.float32, device=DEV)
    L._check(L.load().aurora_hip_zero_words(w[1:].data_ptr(), n, L._stream()))
    torch.cuda.synchronize()
    got = w.cpu()
    assert got[0].item() == 1.0 and bool((got[1:1 + n] == 0).all())
    assert torch.equal(got[1 + n:], torch.arange(2 + n, 67, dtype=torch.float32))


SPLIT_PLANTS = [0.0, -0.0, 1e-9, -2e-8, 2.0 ** -25, 3e-8, 7e-5, -1e-3, 0.1, 0.2499, 16383.99, -16383.99, 65504.0 / 64, 70000.0]


@pytest.mark.parametrize("scale", [1.0, 64.0])
@pytest.mark.parametrize("rows", [1, 70, 257])
@pytest.mark.parametrize("K", [32, 96, 512])
def test_split_f16_values_at_the_ends_of_the_fp16_range(K, rows, scale):
    """hi = fp16(s x), lo = fp16(s x - hi), round to nearest even, from rows with a pitch.  Planted: +-0; |x| <= 2^-25, where
    hi is 0 (and lo too: below half the smallest fp16 subnormal); (2^-14, 0.25), where the remainder is an fp16 subnormal;
    16383.99; 65504 / 64 (with s = 64 exactly the largest fp16); and 70000, past the range: hi = +inf and lo = fp16(70000 - inf)
    = -inf, so that hi + lo is NaN -- a pair out of range does not saturate, it poisons every sum it enters."""
    g = torch.Generator().manual_seed(K + rows)
    base = torch.randn(rows, K + 4, generator=g) * 3
    plants = torch.tensor(SPLIT_PLANTS)
    flat = base[:, :K]
    for r in {0, rows - 1}:
        flat[r, :plants.numel()] = plants
        flat[r, K - plants.numel():] = -plants
    x = base.to(DEV)[:, :K]
    assert x.stride(0) == K + 4
    hi, lo = unsplit(L.split_f16(x, scale=scale).cpu())
    xs = base[:, :K] * scale
    ref_hi = xs.half().float()
    ref_lo = (xs - ref_hi).half().float()
    assert torch.equal(_bits(hi), _bits(ref_hi)) and torch.equal(_bits(lo), _bits(ref_lo))
    c = SPLIT_PLANTS.index(70000.0)
    assert hi[0, c].item() == INF and lo[0, c].item() == -INF
    tiny = SPLIT_PLANTS.index(1e-9)
    if scale == 1.0:
        assert hi[0, tiny].item() == 0.0 and lo[0, tiny].item() == 0.0 and hi[0, SPLIT_PLANTS.index(2.0 ** -25)].item() == 0.0
    else:
        top = SPLIT_PLANTS.index(65504.0 / 64)
        assert hi[0, top].item() == 65504.0 and lo[0, top].item() == 0.0
