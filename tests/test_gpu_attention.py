"""window_attention (csrc/attention.hip) against the fp64 reference of tests/attention_reference.py, on hand-built tables:
every window size on both sides of every tile count, padded positions with and without a bias, group tables, bands that
store fewer rows than they read (L_out < L), head planes with B > 1, wide rows, and item counts on both sides of the XCD
remap's thresholds.

  window_attention_f32                 one thread per query; every case below that lists f32
  window_attention_bf16<false, 1>      N != 144: run-time tile counts, the -inf patch of a ragged last tile, 16-byte stores
  window_attention_bf16<true, 2>       N == 144: constant tile counts, whole-row stores through the i ^ 8 partner lane

Every launch writes into a NaN-filled buffer with guard rows behind B * L_out.  A case asserts: the error per (token, head)
over the natural scale (max |v| over the keys of the token's window) stays within the tolerance of attention_reference
(F32_TOL / BF16_TOL: multiples of what a CPU fp32 evaluation / a CPU model of the bf16 rounding points shows, not of what
the kernels show); every stored row is finite; no other row was touched; a second launch gives the same bits.  bf16 inputs are
rounded first and the reference sees the rounded values.  tests/test_attention_reference.py shows that these inputs tell
a wrong mask, a dropped or admitted key, a wrong padding row, ignored halo keys, a half row of the partner query, the
wrong batch element, head or item and a misplaced 8-column piece from the right result by >= 10 x BF16_TOL.
"""
import pytest
import torch

from tests import attention_reference as R
from tests.device_buffers import DEV, NAN, same_bits

pytestmark = pytest.mark.gpu

DTYPE_PARAMS = ["f32", "bf16"]


def lib():
    from aurora_amd.engine import lib as L

    L.load()
    return L


def check(case: R.Case, dtype: str):
    """One case in one type, in every layout the case names (fp32: rows only -- head planes are a bf16 layout)."""
    if dtype not in case.dtypes:
        return
    L = lib()
    p = R.problem(case, dtype)
    ref, written, scale = R.attention_ref(*p.args())
    tol = R.f32_tol(case.inputs) if dtype == "f32" else R.BF16_TOL
    rows = p.B * p.L_out
    guard = p.L - p.L_out + 2        # where a halo row of the last batch element would land if it were stored
    tok_d = p.tok.to(DEV)
    grp_d = None if p.grp is None else p.grp.to(DEV)
    bias_d = None if p.bias is None else p.bias.to(DEV)
    for layout in (case.layouts if dtype == "bf16" else ("rows",)):
        planes = layout == "planes"
        qkv_d = (R.to_planes(p.qkv, p.heads) if planes else p.qkv).to(DEV).contiguous()
        bufs = [torch.full((rows + guard, p.D), NAN, dtype=p.qkv.dtype, device=DEV) for _ in range(2)]
        for buf in bufs:
            L.window_attention(qkv_d, bias_d, buf[:rows], tok_d, grp_d, p.B, p.L, p.D, p.heads, L_out=p.L_out, planes=planes)
        torch.cuda.synchronize()
        what = (case.id, dtype, layout)
        out = bufs[0][:rows].reshape(p.B, p.L_out, p.D).cpu()
        assert bool(torch.isfinite(out[written]).all()), what
        err = R.worst(R.row_error(out, ref, scale)[written])
        print(f"{case.id} {dtype} {layout}: row error {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, (what, err, tol)
        assert bool(torch.isnan(out[~written]).all()) and bool(torch.isnan(bufs[0][rows:]).all()), what
        assert same_bits(bufs[0], bufs[1]), what


@pytest.mark.parametrize("N", R.WINDOW_SIZES)
@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_window_sizes(dtype, N):
    """nt = ceil(N / 16) = 1..9 against the three waves (`qt < nt`, `break`), a ragged last tile with 1, 2, 3, 4, 15 live
    keys (the -inf patch; N <= 3: inside the first 4-key group of lane group 0), whole tiles without a patch (16, 32, 48,
    64, 96, 128), nine tiles without FULL (129, 143) and FULL (144).  Padded positions at either end, a whole padded
    tile, a window of padding but for one position; each with a bias and without one (padded rows are zero); and the
    low-score inputs, on which a zero key admitted by mistake takes most of the weight."""
    for case in R.window_size_cases(N):
        check(case, dtype)


@pytest.mark.parametrize("N", R.GROUP_SIZES)
@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_groups(dtype, N):
    """No group table; a table that is uniform in every window (bf16: the `differs` shortcut leaves `masked` off); mixed
    groups with 27 among them; and scores of 128 on the keys of one group, where -100 x (group difference) and -inf
    part ways with the literal -100."""
    for case in R.group_cases(N):
        check(case, dtype)


@pytest.mark.parametrize("N", R.GROUP_SIZES)
@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_band_stores_fewer_rows_than_it_reads(dtype, N):
    """L_out < L, rows and planes: halo rows are keys of owned queries and are never stored.  Within one 16-query tile: i
    owned and i ^ 8 a halo row, the reverse, i padded and its partner owned, the reverse, a pair of halo rows; a whole
    tile and a whole window of halo rows (N = 144: the partner-lane stores of WIDE = 2 under `tq_p` / `live_p`)."""
    for case in R.halo_cases(N):
        check(case, dtype)


@pytest.mark.parametrize("N", R.WIDE_SIZES)
@pytest.mark.parametrize("heads", R.PLANE_HEADS)
def test_head_planes(heads, N):
    """(heads, B * L, 3, 64) with B = 2: `b * L * row_stride + h * plane_stride` for b > 0, against fp64 and not against
    the row layout of the same kernel."""
    for case in R.plane_cases(heads, N):
        check(case, "bf16")


@pytest.mark.parametrize("N", R.WIDE_SIZES)
@pytest.mark.parametrize("heads", R.ROW_HEADS)
@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_wide_rows(dtype, heads, N):
    """D = 320 and 2048 in the row layout: column offsets up to 3 x 2048."""
    for case in R.wide_row_cases(heads, N):
        check(case, dtype)


@pytest.mark.parametrize("N", R.PEAKED_SIZES)
@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_peaked_softmax(dtype, N):
    """Scores of standard deviation ~30: almost one-hot weights, exp2 arguments down to several hundred below zero."""
    for case in R.peaked_cases(N):
        check(case, dtype)


@pytest.mark.parametrize("items", sorted(R.ITEMS_ROWS))
def test_item_order_rows(items):
    """Below the threshold of the row layout (plain order), on it, and above it with remainders 3, 4 and 7 by the eight
    XCDs.  The counts follow `xcd_order` in aurora_hip_window_attention_planes and must move with it."""
    for case in R.item_cases("rows", items):
        check(case, "bf16")


@pytest.mark.parametrize("items", sorted(R.ITEMS_PLANES))
def test_item_order_planes(items):
    """As above for head planes (threshold 3000), where items decode head-major."""
    for case in R.item_cases("planes", items):
        check(case, "bf16")


@pytest.mark.parametrize("layout", ["rows", "planes"])
def test_item_order_full_windows(layout):
    """N = 144 above the threshold: 6004 / 3004 items of 48 live tokens and 96 padded positions each."""
    for case in R.item_cases_144(layout):
        check(case, "bf16")
