"""layernorm, layernorm_split, merge_ln and split_ln (csrc/norm.hip) against the fp64 references of tests/norm_reference.py,
at every register-tile instantiation and on both sides of every boundary between two of them:

  layernorm_f32_kernel<T, NC, PRE>   NC = 1|2|4|8|16 for D <= 256|512|1024|2048|4096, rows of 4-feature pieces, the last
                                     chunk of 64 pieces partly masked unless D % 256 == 0; bf16 takes PRE (residual row
                                     prefetched) when there is a residual and M <= 40 x CUs
  merge_ln_kernel / split_ln_kernel<T, MAXC>   MAXC = 1|2|4|8 for a row of <= 512|1024|2048|4096, 8-feature pieces

fp32 results are judged ROW BY ROW: max_j |out - ref| over the row's natural scale max_j(|LN gain| + |shift| + |res|)
must stay within norm_reference.F32_TOL.  bf16 results are held to the fp32 result of the same launch (or of the fp32
launch on the same rounded input), rounded once, bit for bit.  tests/test_norm_reference.py shows that these inputs tell
a one-pass variance, statistics without the merge padding, a (dw, dh) segment order, a crop from the wrong end, an
ignored res_mod and a misplaced 8-feature piece from the right result by >= 100 x the tolerance.
"""
import pytest
import torch

from tests import norm_reference as R
from tests.device_buffers import DEV, NAN, Padded, same_bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_PARAMS = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")]


def lib():
    from aurora_amd.engine import lib as L

    L.load()
    return L


def assert_rows(out, ref, scale, what):
    err = R.worst(R.row_error(out, ref, scale))
    assert err <= R.F32_TOL, (what, err)


# ------------------------------------------------------------------------------------------
# layernorm
# ------------------------------------------------------------------------------------------
# (name, gain, shift, residual: None | "full" | "mod")
OPERAND_FORMS = [("none", False, False, None), ("gain", True, False, None), ("shift", False, True, None),
                 ("all, full residual", True, True, "full"), ("all, res_mod", True, True, "mod")]
LD_Y, LD_RES, LD_F32, LD_T = 8, 16, 24, 32   # four different leading dimensions: D + these, all 16-byte multiples


def check_layernorm(dtype, D, M, eps=1e-5, y=None):
    """Every operand form and output form of one (dtype, D, M) against fp64, on views into wider NaN-filled buffers."""
    L = lib()
    y0, gain, shift, res, res5 = R.ln_inputs(M, D, dtype)
    y0 = y0 if y is None else y.to(dtype)
    yp = Padded(M, D, LD_Y, dtype, y0)
    g_dev, s_dev = gain.to(DEV), shift.to(DEV)
    results = {}
    for name, has_gain, has_shift, residual in OPERAND_FORMS:
        r_host = {None: None, "full": res, "mod": res5}[residual]
        res_mod = R.RES_MOD if residual == "mod" else 0
        ref, scale = R.layernorm_ref(y0, gain if has_gain else None, shift if has_shift else None, r_host, res_mod, eps)
        rp = None if r_host is None else Padded(r_host.shape[0], D, LD_RES, fill=r_host)
        of, ot = Padded(M, D, LD_F32), Padded(M, D, LD_T, dtype)
        L.layernorm(yp.view, g_dev if has_gain else None, s_dev if has_shift else None, res=None if rp is None else rp.view,
                    res_mod=res_mod, out_f32=of.view, out_t=ot.view, eps=eps)
        torch.cuda.synchronize()
        what = (name, str(dtype), D, M)
        assert_rows(of.view, ref, scale, what)
        # out_t: the fp32 result itself / rounded to bf16 once
        assert same_bits(ot.view, of.view.to(dtype)), what
        assert yp.untouched() and of.untouched() and ot.untouched() and (rp is None or rp.untouched()), what
        results[name] = (of.view.clone(), ot.view.clone(), rp, ref, scale)

    # either output alone writes what the launch with both wrote
    f_both, t_both, rp, ref, scale = results["all, full residual"]
    of, ot = Padded(M, D, LD_F32), Padded(M, D, LD_T, dtype)
    L.layernorm(yp.view, g_dev, s_dev, res=rp.view, out_f32=of.view, eps=eps)
    L.layernorm(yp.view, g_dev, s_dev, res=rp.view, out_t=ot.view, eps=eps)
    torch.cuda.synchronize()
    assert same_bits(of.view, f_both) and same_bits(ot.view, t_both), (str(dtype), D, M)
    assert of.untouched() and ot.untouched() and rp.untouched()
    # in place on the residual stream: out_f32 is res
    ot = Padded(M, D, LD_T, dtype)
    L.layernorm(yp.view, g_dev, s_dev, res=rp.view, out_f32=rp.view, out_t=ot.view, eps=eps)
    torch.cuda.synchronize()
    assert same_bits(rp.view, f_both) and same_bits(ot.view, t_both), (str(dtype), D, M)
    assert rp.untouched() and ot.untouched() and yp.untouched()
    # in place on the input: out_f32 is y (fp32 rows only)
    if dtype == torch.float32:
        ref, scale = R.layernorm_ref(y0, gain, shift, eps=eps)
        L.layernorm(yp.view, g_dev, s_dev, out_f32=yp.view, eps=eps)
        torch.cuda.synchronize()
        assert_rows(yp.view, ref, scale, ("in place on y", D, M))
        assert yp.untouched()


@pytest.mark.parametrize("M", R.LN_ROWS)           # a single row, a partial block of 4 rows, a block and a half, many
@pytest.mark.parametrize("D", R.LN_WIDTHS)
@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_layernorm(dtype, D, M):
    """fp32: layernorm_f32_kernel<float, NC>; bf16 (M <= 40 x CUs): <bf16_t, NC> without a residual, <bf16_t, NC, PRE>
    with one (NC = 16 has no PRE form)."""
    check_layernorm(dtype, D, M)


@pytest.mark.parametrize("D", [264, 1032])
def test_layernorm_bf16_rows_beyond_the_prefetch_threshold(D):
    """M > 40 x CUs: bf16 rows WITH a residual take the kernel that fetches it after the statistics."""
    M = 40 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    check_layernorm(torch.bfloat16, D, M)


@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_layernorm_eps_dominates_a_small_variance(dtype):
    """Rows of spread 1e-2 (variance ~3e-5) with eps = 1e-3: eps left out, or the default taken, is 30 x off."""
    check_layernorm(dtype, 264, 1001, eps=1e-3, y=R.eps_inputs(1001, 264))


@pytest.mark.parametrize("D", R.LARGE_MEAN_WIDTHS)
@pytest.mark.parametrize("c", R.LARGE_MEANS)
def test_layernorm_statistics_under_a_large_mean(c, D):
    """Rows c + z, z uniform in +-1: a variance taken as E[x^2] - mean^2 loses log2(c^2) bits, the two-pass statistics the
    file header promises lose log2(c).  The bound is not a constant: it is norm_reference.LARGE_MEAN_FACTOR = 4 x the
    worst per-row error of torch's CPU fp32 layer_norm on the same rows against fp64 (the kernel sums in another order;
    a 64-lane tree against a cascaded sum is worth a small constant factor at most).  Measured, worst row of 1001:

        c     D      CPU fp32 layer_norm   bound     this kernel
        1e2   264    1.6e-5                6.5e-5    1.5e-5
        1e2   2048   1.2e-5                4.9e-5    9.8e-6
        1e4   264    1.8e-3                7.2e-3    1.8e-3
        1e4   2048   1.7e-3                7.0e-3    1.2e-3

    The one-pass form misses these bounds by 114 x, 119 x, 2.8e4 x and 2.7e4 x (tests/test_norm_reference.py)."""
    L = lib()
    y = R.large_mean_inputs(c, D)
    bound, measured = R.large_mean_bound(y)
    ref, scale = R.layernorm_ref(y)
    out = torch.full((y.shape[0], D), NAN, device=DEV)
    L.layernorm(y.to(DEV), None, None, out_f32=out)
    torch.cuda.synchronize()
    err = R.worst(R.row_error(out, ref, scale))
    print(f"large mean c={c:g} D={D}: CPU fp32 layer_norm {measured:.3e}, bound {bound:.3e}, kernel {err:.3e}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("D", [256, 264, 2048])
@pytest.mark.parametrize("dtype", DTYPE_PARAMS)
def test_layernorm_constant_rows(dtype, D):
    """y == 0.75 everywhere.  Sums of a dyadic value over a power-of-two width are exact in any order, so at D = 256 and 2048
    the mean is 0.75, every centred value 0 and out == shift + res EXACTLY (the fp32 sum, rounded once).  At D = 264 the
    mean is sum x fl(1/264), within 2^-23 relative of c, so |LN| <= |c| 2^-23 eps^-1/2 and
    |out - shift - res| <= |c| 2^-23 eps^-1/2 |gain| per element.  (That bounds the LN term; the two fp32 additions round by
    <= 2^-23 (|shift| + |res|) <= 2.4e-7 more, which the bound, 2.8e-5 |gain|, covers because the gains of this test are drawn
    from +-[0.5, 2] -- a gain near zero would leave a bound of zero for a sum that is rounded.)"""
    L = lib()
    M, c, eps = 7, 0.75, 1e-5
    y = torch.full((M, D), c, dtype=dtype, device=DEV)
    sign = torch.where(R.rnd(D, seed=21) < 0, -1.0, 1.0)
    gain = (sign * (1.25 + 0.75 * R.rnd(D, seed=22))).float()
    shift, res = R.rnd(D, seed=23).float(), R.rnd(M, D, seed=24).float()
    assert gain.abs().min().item() >= 0.5
    out, bare = torch.full((M, D), NAN, device=DEV), torch.full((M, D), NAN, device=DEV)
    L.layernorm(y, gain.to(DEV), shift.to(DEV), res=res.to(DEV), out_f32=out, eps=eps)
    L.layernorm(y, gain.to(DEV), None, out_f32=bare, eps=eps)
    torch.cuda.synchronize()
    if D != 264:
        assert torch.equal(out.cpu(), shift + res) and torch.equal(bare.cpu(), torch.zeros(M, D))
    else:
        bound = abs(c) * 2.0 ** -23 * eps ** -0.5 * gain.double().abs()
        assert bool(((out.double().cpu() - shift.double() - res.double()).abs() <= bound).all())
        assert bool((bare.double().cpu().abs() <= bound).all())


# ------------------------------------------------------------------------------------------
# layernorm_split: output and residual in the fp16-pair layout
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.SPLIT_LN_ROWS)
@pytest.mark.parametrize("D", R.SPLIT_LN_WIDTHS)   # 544, 2080: a ragged last chunk; 32: the lane-pair exchange on 8 lanes only
def test_layernorm_split(D, M):
    """Pair-layout output with ld_split = D + 32, pair-layout residual with ldr = D + 64 read cyclically (res_mod = 5):
    bit for bit split_f16 of the plain launch's result, and the plain launch on high half + remainder of the residual."""
    L = lib()
    y, gain, shift, _, res5 = R.ln_inputs(M, D, torch.float32)
    y_dev, g_dev, s_dev, r_dev = y.to(DEV), gain.to(DEV), shift.to(DEV), res5.to(DEV)
    ref, scale = R.layernorm_ref(y, gain, shift, res5, R.RES_MOD)
    plain = torch.full((M, D), NAN, device=DEV)
    L.layernorm(y_dev, g_dev, s_dev, res=r_dev, res_mod=R.RES_MOD, out_f32=plain)
    both, sp, only = Padded(M, D, 8), Padded(M, D, 32), Padded(M, D, 32)
    L.layernorm(y_dev, g_dev, s_dev, res=r_dev, res_mod=R.RES_MOD, out_f32=both.view, out_t=sp.view, split_t=True)
    L.layernorm(y_dev, g_dev, s_dev, res=r_dev, res_mod=R.RES_MOD, out_t=only.view, split_t=True)
    torch.cuda.synchronize()
    assert_rows(plain, ref, scale, ("plain", D, M))
    want = L.split_f16(plain)
    assert same_bits(both.view, plain) and same_bits(sp.view, want) and same_bits(only.view, want)
    assert both.untouched() and sp.untouched() and only.untouched()

    # the residual in the pair layout is worth high half + remainder
    pairs = Padded(R.RES_MOD, D, 64)
    L.split_f16(r_dev, out=pairs.view)
    halves = pairs.view.contiguous().view(torch.float16).view(R.RES_MOD, D // 32, 2, 32)
    hi_lo = (halves[:, :, 0].float() + halves[:, :, 1].float()).reshape(R.RES_MOD, D)
    exact = torch.full((M, D), NAN, device=DEV)
    L.layernorm(y_dev, g_dev, s_dev, res=hi_lo, res_mod=R.RES_MOD, out_f32=exact)
    from_pairs, sp2 = Padded(M, D, 8), Padded(M, D, 32)
    L.layernorm(y_dev, g_dev, s_dev, res=pairs.view, res_mod=R.RES_MOD, out_f32=from_pairs.view, out_t=sp2.view,
                split_t=True, split_res=True)
    torch.cuda.synchronize()
    assert same_bits(from_pairs.view, exact) and same_bits(sp2.view, L.split_f16(exact))
    assert from_pairs.untouched() and sp2.untouched() and pairs.untouched()
    ref_pairs, scale_pairs = R.layernorm_ref(y, gain, shift, hi_lo, R.RES_MOD)
    assert_rows(from_pairs.view, ref_pairs, scale_pairs, ("pair residual", D, M))


# ------------------------------------------------------------------------------------------
# merge_ln / split_ln
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", R.MERGE_GRIDS)     # rows = 6 H2 W2: 72, 120, 18, 18, 6 (the last three: no multiple of 4)
@pytest.mark.parametrize("D", R.MERGE_WIDTHS)
def test_merge_ln(D, H, W):
    """merge_ln_kernel<float | bf16_t, MAXC>, MAXC = 1|2|4|8 for 4D <= 512|1024|2048|4096."""
    L = lib()
    B, C = R.BC
    x, w, b = R.merge_inputs(H, W, D)
    ref, scale = R.merge_ln_ref(x, w, b, B, C, H, W, D)
    rows = ref.shape[0]
    out = {dt: torch.full((rows + 1, 4 * D), NAN, dtype=dt, device=DEV) for dt in DTYPES}
    for dt in DTYPES:
        L.merge_ln(x.to(DEV), w.to(DEV), b.to(DEV), out[dt][:rows], B, C, H, W, D)
    torch.cuda.synchronize()
    assert_rows(out[torch.float32][:rows], ref, scale, (D, H, W))
    assert same_bits(out[torch.bfloat16][:rows], out[torch.float32][:rows].bfloat16())
    assert all(bool(torch.isnan(o[rows:]).all()) for o in out.values())


@pytest.mark.parametrize("crop", R.CROPS)
@pytest.mark.parametrize("H,W", R.SPLIT_GRIDS)     # H = 1 with crop_h = 1: a single output row per (b, c)
@pytest.mark.parametrize("Dq", R.SPLIT_WIDTHS)
def test_split_ln(Dq, H, W, crop):
    """split_ln_kernel<float | bf16_t, MAXC>, MAXC = 1|2|4|8 for Dq <= 512|1024|2048|4096.  The fp32 kernel runs on fp32
    inputs and on the bf16-rounded ones; the bf16 kernel must give the latter result rounded once."""
    L = lib()
    B, C = R.BC
    w, b = R.split_inputs(H, W, Dq, torch.float32)[1:]
    w_dev, b_dev = w.to(DEV), b.to(DEV)
    rows = B * C * (2 * H - crop[0]) * (2 * W - crop[1])
    f32_of = {}
    for dt in DTYPES:
        y = R.split_inputs(H, W, Dq, dt)[0]
        ref, scale = R.split_ln_ref(y, w, b, B, C, H, W, Dq, *crop)
        assert ref.shape[0] == rows
        out = torch.full((rows + 1, Dq), NAN, device=DEV)
        L.split_ln(y.float().to(DEV), w_dev, b_dev, out[:rows], B, C, H, W, Dq, *crop)
        torch.cuda.synchronize()
        assert_rows(out[:rows], ref, scale, (str(dt), Dq, H, W, crop))
        assert bool(torch.isnan(out[rows:]).all())
        f32_of[dt] = out[:rows]
    y16 = R.split_inputs(H, W, Dq, torch.bfloat16)[0]
    out16 = torch.full((rows + 1, Dq), NAN, dtype=torch.bfloat16, device=DEV)
    L.split_ln(y16.to(DEV), w_dev, b_dev, out16[:rows], B, C, H, W, Dq, *crop)
    torch.cuda.synchronize()
    assert same_bits(out16[:rows], f32_of[torch.bfloat16].bfloat16())
    assert bool(torch.isnan(out16[rows:]).all())


# ------------------------------------------------------------------------------------------
# argument checks: nothing is launched
# ------------------------------------------------------------------------------------------
def test_norm_argument_checks():
    L = lib()
    M = 6

    def buf(cols, dtype=torch.float32):
        return torch.full((M, cols), NAN, dtype=dtype, device=DEV)

    def rejected(message, call, *outputs):
        with pytest.raises(ValueError, match=message) as e:
            call()
        assert "(code -1)" in str(e.value) and message in L.load().aurora_hip_last_error().decode()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outputs)

    vec = torch.ones(4200, device=DEV)
    ones = lambda cols, dtype=torch.float32: torch.ones((M, cols), dtype=dtype, device=DEV)   # noqa: E731
    o = buf(4200)
    rejected("must be a multiple of 8", lambda: L.layernorm(ones(12), vec, vec, out_f32=o[:, :12]), o)
    rejected("must be a multiple of 8, <= 4096", lambda: L.layernorm(ones(4104), vec, vec, out_f32=o[:, :4104]), o)
    rejected("unaligned input rows", lambda: L.layernorm(ones(66)[:, :64], vec, vec, out_f32=o[:, :64]), o)
    rejected("unaligned input rows", lambda: L.layernorm(ones(68, torch.bfloat16)[:, :64], vec, vec, out_f32=o[:, :64]), o)
    rejected("no output", lambda: L.layernorm(ones(64), vec, vec))
    sp = buf(96)
    rejected("must be a multiple of 32", lambda: L.layernorm(ones(40), vec, vec, out_t=sp[:, :40], split_t=True), sp)
    sp = buf(72)
    rejected("pair-layout output stride", lambda: L.layernorm(ones(64), vec, vec, out_t=sp[:, :64], split_t=True), sp)
    # a pair-layout residual without a residual (the Python wrapper asserts this itself: the C entry point directly)
    y, out = ones(64), buf(64)
    code = L.load().aurora_hip_layernorm_split(y.data_ptr(), 64, None, None, None, 64, 0, 1, out.data_ptr(), 64, None, 0,
                                               M, 64, 1e-5, None)
    torch.cuda.synchronize()
    assert code == -1 and "pair-layout residual" in L.load().aurora_hip_last_error().decode()
    assert bool(torch.isnan(out).all())

    B, C = R.BC
    mo = torch.full((B * C, 4 * 1032), NAN, device=DEV)
    rejected("4D <= 4096", lambda: L.merge_ln(torch.ones(B * C * 1032, device=DEV), vec, vec, mo, B, C, 1, 1, 1032), mo)
    so = torch.full((B * C * 2 * 4, 8), NAN, device=DEV)
    rejected("crop must be 0 or 1", lambda: L.split_ln(torch.ones(B * C * 4 * 32, device=DEV), vec, vec, so, B, C, 2, 2, 8, 2, 0), so)

    # no rows: fine, and nothing written (a zero-row tensor has no address to pass: the C entry point directly)
    y, out = ones(64), buf(64)
    for dtype_code in (L.F32, L.BF16):
        assert L.load().aurora_hip_layernorm(y.data_ptr(), 64, vec.data_ptr(), vec.data_ptr(), None, 0, 0, out.data_ptr(), 64,
                                             None, 0, 0, 64, 1e-5, dtype_code, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
