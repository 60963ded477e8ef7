"""patchify, unpatchify and assemble_tokens (csrc/embed.hip) against the fp64 references of tests/embed_reference.py, in
every kernel form and behind every condition that sends a call from one form to another.

patchify -- three forms:
  patchify_kernel               P = 4, fp32 output, out / Kpad / k_offset multiples of 4 floats, every source 16-byte
                                aligned with unit stride_w and the other strides % 4 == 0, n_vars T <= 32.  Reached by
                                test_patchify_vector_form (Wp on both sides of the 8-patch lane groups and of the 32-patch
                                run; blocks of 64, 192 and 1024 threads), test_patchify_in_several_calls[vector] and
                                test_patchify_absmax[vector].
  patchify_cols_kernel<float>   everything else in fp32: P = 3 and 10 in test_patchify_any_p_form, and at P = 4 each
                                fallback condition alone in test_patchify_leaves_the_vector_form -- source pointer off by
                                one float, stride_h % 4 != 0, stride_w = 2, Kpad % 4 != 0, n_vars T = 33.
  patchify_cols_kernel<bf16>    every bf16 call: test_patchify_any_p_form launches it next to the fp32 any-P form on the
                                same input (at P = 4 the fp32 launch is pushed off the vector form by a source pointer one
                                float off) and wants the fp32 operand rounded once, bit for bit.
  Columns: fewer than one 256-column chunk (P = 3, 4 variables), two chunks (P = 10, 2 variables), exactly one (P = 4,
  8 variables) with and without K padding.

unpatchify -- two forms:
  unpatchify_kernel<4>          P = 4 and y, ldy, every dst, col0, lvl_stride, and of the hooks in use mod_col0, prev and
                                its strides, angle_col0, dens_col0, mask and mask_sh all multiples of 4 floats.  Reached by
                                test_unpatchify_vector_form and test_unpatchify_level_conditioned_heads[4].
  unpatchify_kernel<1>          everything else: P = 3 and 10 in test_unpatchify_any_p_form (image rows of 3, 255, 258 and
                                260 pixels: one 256-pixel chunk and the step past it), and at P = 4 each of the twelve
                                fallback conditions alone in test_unpatchify_leaves_the_vector_form.
  Both forms run the same variable mix (embed_reference.UNPATCH_MIX): every hook combination in both.

assemble_tokens -- assemble_kernel<float> (no out_t) and <bf16_t>; test_assemble_tokens_grid_stride_loop passes the
16384-block cap, so that the loop takes a second trip.

Every output sits in a NaN-filled buffer with guard rows or words that must still be NaN afterwards, inputs must be
bit-unchanged, and every element is held to |out - ref| <= tolerance x scale with equal NaN positions
(embed_reference.ratios; the tolerances are derived or measured there).  tests/test_embed_reference.py shows that these
inputs tell every planted fault from the right result by >= 100 x the tolerance.
"""
import math

import pytest
import torch

from tests import embed_reference as R
from tests.device_buffers import DEV, NAN, same_bits

pytestmark = pytest.mark.gpu

B, T, HP = 2, 2, 3
POISON = 7.0e7          # fills the parts of a source buffer that no launch may read
GUARD = 16              # NaN words in front of and behind every unpatchify field


def lib():
    from aurora_amd.engine import lib as L

    L.load()
    return L


def assert_close(out, ref, scale, kind, tols, what, names):
    """Every element within its tolerance; prints the worst error per kind in units of u x scale (what the MEASURED
    constants of embed_reference record) before asserting."""
    per_kind = R.worst_by_kind(out, ref, scale, kind, len(names))
    print("MEASURE", what, " ".join(f"{n}={w:.3f}u" for n, w in zip(names, per_kind)))
    worst = float(R.ratios(out, ref, scale, kind, tols).max())
    assert worst <= 1.0, (what, "worst |out - ref| / (tol x scale)", worst, per_kind)


PATCH_KINDS = ("linear", "exact", "t2", "trig")
UNPATCH_KINDS = ("plain", "diff", "angle")


# ------------------------------------------------------------------------------------------
# patchify
# ------------------------------------------------------------------------------------------
class PatchSources:
    """The variables of embed_reference.patch_inputs on the device, each a cropped view (one latitude row more than the
    patches cover) of a POISON-filled buffer: `lead` floats in front, rows `pitch_extra` floats longer, `extra_rows` more
    rows per plane, every `step_w`-th float a pixel."""

    def __init__(self, L, vars, H, lead=0, pitch_extra=0, extra_rows=0, step_w=1):
        self.bufs, self.descs, self.keep = [], [], []
        for v in vars:
            x = v["x"]
            shape = list(x.shape)
            shape[-2] += extra_rows
            shape[-1] = shape[-1] * step_w + pitch_extra
            buf = torch.full((lead + math.prod(shape),), POISON, device=DEV)
            view = buf[lead:].view(shape)[..., :x.shape[-2], :x.shape[-1] * step_w:step_w]
            view.copy_(x)
            crop = view[..., :H, :]
            strides = crop.stride() if x.dim() == 5 else (0, 0, 0) + tuple(crop.stride())
            loc, inv = v["loc"].to(DEV), v["inv"].to(DEV)
            self.descs.append(L.PatchVar(crop.data_ptr(), *strides, loc.data_ptr(), inv.data_ptr(), v["transform"],
                                         v["tw0"], v["tw1"], v["tb"]))
            self.bufs.append(buf)
            self.keep += [loc, inv]
        self.before = [b.clone() for b in self.bufs]

    def unchanged(self):
        return all(same_bits(a, b) for a, b in zip(self.bufs, self.before))


def patch_k(vars, P):
    return len(vars) * T * P * P


def launch_patchify(L, src, vars, n_lvl, Wp, P, Kpad, dtype=torch.float32, absmax=None, t=T):
    """One call for all variables into the leading rows of a NaN-filled operand two rows longer."""
    rows = n_lvl * B * HP * Wp
    buf = torch.full((rows + 2, Kpad), NAN, dtype=dtype, device=DEV)
    L.patchify(src.descs, buf[:rows], 0, len(vars) * t * P * P, B, t, n_lvl, HP, Wp, P, absmax=absmax)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[rows:]).all()) and src.unchanged()
    return buf[:rows]


def check_patchify(vars, n_lvl, Wp, P, pad, what, t=T, **layout):
    """fp32 launch against fp64; returns (operand, sources)."""
    L = lib()
    K = len(vars) * t * P * P
    src = PatchSources(L, vars, HP * P, **layout)
    out = launch_patchify(L, src, vars, n_lvl, Wp, P, K + pad, t=t)
    assert_close(out[:, :K], *R.patchify_ref(vars, B, t, n_lvl, HP, Wp, P), R.PATCH_TOL, what, PATCH_KINDS)
    assert bool((out[:, K:] == 0).all()), what
    return out, src


@pytest.mark.parametrize("fill", ["mix", 1, 3, 32])
@pytest.mark.parametrize("Wp", [1, 7, 8, 9, 31, 32, 33])
def test_patchify_vector_form(Wp, fill):
    """patchify_kernel.  `mix`: one variable of each transform 0-6 and a static plane (stride_b = stride_t = stride_c = 0)
    with T = 2, at three levels and at one.  1 | 3 | 32 pieces (n_vars T): a 64-thread block, a partly filled block of 192,
    the full 1024 (16 variables, T = 2)."""
    if fill == "mix":
        for n_lvl in (3, 1):
            vars = R.patch_inputs(R.patch_transforms(7), B, T, n_lvl, HP, Wp, 4, static=True, seed=Wp)
            check_patchify(vars, n_lvl, Wp, 4, 32, ("vector", Wp, fill, n_lvl))
    else:
        n_vars, t = {1: (1, 1), 3: (3, 1), 32: (16, 2)}[fill]
        vars = R.patch_inputs(R.patch_transforms(n_vars), B, t, 3, HP, Wp, 4, seed=Wp)
        check_patchify(vars, 3, Wp, 4, 32, ("vector", Wp, fill), t=t)


ANY_P_CASES = [(P, Wp, "mix") for P in (3, 10, 4) for Wp in (1, 15, 16, 17, 37)] + \
    [(3, 17, "4 variables, 72 columns"), (10, 17, "2 variables, 400 columns"),
     (4, 17, "8 variables, 256 columns, Kpad = K"), (4, 17, "8 variables, 256 columns, Kpad = K + 32")]


@pytest.mark.parametrize("P,Wp,columns", ANY_P_CASES)
def test_patchify_any_p_form(P, Wp, columns):
    """patchify_cols_kernel<float> against fp64, and <bf16> = that fp32 operand rounded once.  Wp on both sides of the
    16-patch span; at P = 4 the fp32 launch reads its sources one float off 16-byte alignment, which the vector form
    refuses."""
    L = lib()
    layout = {"lead": 1} if P == 4 else {}
    for n_lvl in ((3, 1) if columns == "mix" else (3,)):
        if columns == "mix":
            vars, pad = R.patch_inputs(R.patch_transforms(7), B, T, n_lvl, HP, Wp, P, static=True, seed=Wp), 32
        else:
            vars = R.patch_inputs(R.patch_transforms(int(columns[0])), B, T, n_lvl, HP, Wp, P, seed=Wp)
            pad = 0 if columns.endswith("Kpad = K") else 32
        K = patch_k(vars, P)
        assert columns == "mix" or str(K) in columns
        out, src = check_patchify(vars, n_lvl, Wp, P, pad, ("any-P", P, Wp, columns, n_lvl), **layout)
        out16 = launch_patchify(L, src, vars, n_lvl, Wp, P, K + pad, torch.bfloat16)
        assert same_bits(out16, out.to(torch.bfloat16)), (P, Wp, columns, n_lvl)


@pytest.mark.parametrize("why", ["source pointer + 1 float", "stride_h % 4 != 0", "stride_w = 2", "Kpad % 4 != 0",
                                 "n_vars T = 33"])
def test_patchify_leaves_the_vector_form(why):
    """P = 4, fp32, one condition of the vector form broken at a time: the any-P kernel must produce the same values."""
    Wp, pad, t, layout = 9, 32, T, {}
    vars = R.patch_inputs(R.patch_transforms(7), B, T, 3, HP, Wp, 4, static=True, seed=50)
    if why == "source pointer + 1 float":
        layout = {"lead": 1}
    elif why == "stride_h % 4 != 0":
        layout = {"pitch_extra": 2, "extra_rows": 1}      # planes of 14 rows x (W + 2): every other stride stays % 4 == 0
    elif why == "stride_w = 2":
        layout = {"step_w": 2}
    elif why == "Kpad % 4 != 0":
        pad = 3
    else:
        t = 3
        vars = R.patch_inputs(R.patch_transforms(11), B, t, 3, HP, Wp, 4, seed=51)
    check_patchify(vars, 3, Wp, 4, pad, ("fallback", why), t=t, **layout)


@pytest.mark.parametrize("form,P,Wp", [("vector", 4, 9), ("any-P", 3, 17)])
def test_patchify_in_several_calls(form, P, Wp):
    """Three calls over the variables [0, 3), [3, 5), [5, 8) of one operand: a call writes its own columns only -- the
    others' and the K padding stay NaN -- and the call that ends at K_total zeroes the padding."""
    L = lib()
    n_lvl = 3
    vars = R.patch_inputs(R.patch_transforms(7), B, T, n_lvl, HP, Wp, P, static=True, seed=60)
    ref, scale, kind = R.patchify_ref(vars, B, T, n_lvl, HP, Wp, P)
    K, per_var = patch_k(vars, P), T * P * P
    src = PatchSources(L, vars, HP * P)
    rows = n_lvl * B * HP * Wp
    buf = torch.full((rows + 2, K + 32), NAN, device=DEV)
    written = torch.zeros(K + 32, dtype=torch.bool)
    for v0, v1 in ((0, 3), (3, 5), (5, 8)):
        L.patchify(src.descs[v0:v1], buf[:rows], v0 * per_var, K, B, T, n_lvl, HP, Wp, P)
        torch.cuda.synchronize()
        written[v0 * per_var:v1 * per_var] = True
        if v1 == len(vars):
            written[K:] = True
        assert bool(torch.isnan(buf[:, ~written.to(DEV)]).all()), (form, v0, v1)
        done = torch.nonzero(written[:K]).flatten()
        assert_close(buf[:rows][:, done.to(DEV)], ref[:, done], scale[:, done], kind[:, done], R.PATCH_TOL,
                     ("several calls", form, v1), PATCH_KINDS)
    assert bool((buf[:rows, K:] == 0).all()) and bool(torch.isnan(buf[rows:]).all()) and src.unchanged()


@pytest.mark.parametrize("form,P,Wp", [("vector", 4, 33), ("any-P", 10, 17)])
def test_patchify_absmax(form, P, Wp):
    """The word afterwards is max(word before, max |finite value written|) exactly, whether it starts below or above the
    data; the NaN that the first variable writes do not touch it; an infinite input makes it inf; the operand is the same
    with and without a word."""
    L = lib()
    n_lvl = 3
    vars = R.patch_inputs(R.patch_transforms(7), B, T, n_lvl, HP, Wp, P, static=True, seed=70)
    K = patch_k(vars, P)
    src = PatchSources(L, vars, HP * P)
    plain = launch_patchify(L, src, vars, n_lvl, Wp, P, K + 32)
    mags = plain[:, :K].abs()
    assert bool(torch.isnan(mags).any())
    data_max = float(torch.where(torch.isnan(mags), torch.zeros_like(mags), mags).max())
    for start in (0.25, 1.0e6):
        assert (start < data_max) == (start == 0.25)
        word = torch.full((1,), start, device=DEV)
        out = launch_patchify(L, src, vars, n_lvl, Wp, P, K + 32, absmax=word)
        assert float(word) == max(start, data_max), (form, start, float(word), data_max)
        assert same_bits(out, plain)
    vars[1]["x"][1, 1, n_lvl - 1, 5, 2] = float("inf")       # transform 1: the clamp keeps +inf
    word = torch.full((1,), 0.25, device=DEV)
    out = launch_patchify(L, PatchSources(L, vars, HP * P), vars, n_lvl, Wp, P, K + 32, absmax=word)
    assert float(word) == math.inf and int(torch.isinf(out).sum()) == 1


# ------------------------------------------------------------------------------------------
# unpatchify
# ------------------------------------------------------------------------------------------
def check_unpatchify(y, vars, n_lvl, Wp, P, what, y_lead=0, dst_lead=0):
    """One call on the device against unpatchify_ref: every variable's field, its guard words, the inputs."""
    L = lib()
    H, W = HP * P, Wp * P
    n = B * n_lvl * H * W
    y_buf = torch.full((y_lead + y.numel(),), POISON, device=DEV)
    y_dev = y_buf[y_lead:].view(y.shape)
    y_dev.copy_(y)
    inputs, fields, descs, keep = [y_buf], [], [], []
    for v in vars:
        buf = torch.full((GUARD + dst_lead + n + GUARD,), NAN, device=DEV)
        field = buf[GUARD + dst_lead:GUARD + dst_lead + n]
        loc, scale, inv = v["loc"].to(DEV), v["scale"].to(DEV), v["inv"].to(DEV)
        d = L.unpatch_var(field.data_ptr(), loc.data_ptr(), scale.data_ptr(), v["clamp_min0"], v["col0"])
        d.lvl_stride, d.mod_col0, d.angle_col0, d.dens_col0 = v["lvl_stride"], v["mod_col0"], v["angle_col0"], v["dens_col0"]
        d.clamp_max1_levels, d.mask_thresh = v["cap_levels"], v["mask_thresh"]
        if v["prev"] is not None:
            prev = v["prev"].to(DEV)
            d.prev, d.inv_scale = prev.data_ptr() + 4 * v["prev_off"], inv.data_ptr()
            d.prev_sb, d.prev_sc, d.prev_sh = v["prev_sb"], v["prev_sc"], v["prev_sh"]
            inputs.append(prev)
        if v["mask"] is not None:
            mask = v["mask"].to(DEV)
            d.mask, d.mask_sh = mask.data_ptr() + 4 * v["mask_off"], v["mask_sh"]
            inputs.append(mask)
        descs.append(d)
        fields.append((buf, field))
        keep += [loc, scale, inv]
    before = [t.clone() for t in inputs]
    L.unpatchify(y_dev, descs, B, n_lvl, HP, Wp, P)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(inputs, before)), what
    refs = R.unpatchify_ref(y, vars, B, n_lvl, HP, Wp, P)
    for v, (buf, field), (ref, scale, kind) in zip(vars, fields, refs):
        assert bool(torch.isnan(buf[:GUARD + dst_lead]).all() and torch.isnan(buf[-GUARD:]).all()), (what, v["kind"])
        out = field.view(B, n_lvl, H, W)
        assert_close(out, ref, scale, kind, R.UNPATCH_TOL, (what, v["kind"]), UNPATCH_KINDS)
        if v["kind"] == "dir":      # scale 1, loc 0: the field is the direction itself
            assert float(out.min()) >= 0.0 and float(out.max()) <= 360.0, (what, float(out.min()), float(out.max()))


@pytest.mark.parametrize("variables", ["mix", 1, 32])
@pytest.mark.parametrize("Wp", [1, 7, 8, 9, 31, 32, 33])
def test_unpatchify_vector_form(Wp, variables):
    """unpatchify_kernel<4>: the mix of every hook combination at three levels and at one; 1 variable (a 64-thread block)
    and 32 (the full 1024)."""
    if variables == "mix":
        for n_lvl in (3, 1):
            y, vars = R.unpatch_inputs(R.UNPATCH_MIX, B, n_lvl, HP, Wp, 4, seed=Wp)
            check_unpatchify(y, vars, n_lvl, Wp, 4, ("vector", Wp, n_lvl))
    else:
        y, vars = R.unpatch_inputs((["plain", "clamp"] * 16)[:variables], B, 3, HP, Wp, 4, seed=Wp)
        check_unpatchify(y, vars, 3, Wp, 4, ("vector", Wp, variables))


@pytest.mark.parametrize("P,Wp", [(3, 1), (3, 85), (3, 86), (10, 26), (10, 3)])
def test_unpatchify_any_p_form(P, Wp):
    """unpatchify_kernel<1>: image rows of 3, 255, 258, 260 (and 30) pixels -- inside one 256-pixel chunk, and one, two and
    four pixels past it."""
    for n_lvl in (3, 1):
        y, vars = R.unpatch_inputs(R.UNPATCH_MIX, B, n_lvl, HP, Wp, P, seed=Wp)
        check_unpatchify(y, vars, n_lvl, Wp, P, ("any-P", P, Wp, n_lvl))


UNPATCH_FALLBACKS = {
    "y + 1 float": ({}, {"y_lead": 1}), "ldy % 4 != 0": ({"ldy_extra": 5}, {}), "dst + 1 float": ({}, {"dst_lead": 1}),
    "col0 % 4 != 0": ({"pad_before": ("col0",)}, {}), "mod_col0 % 4 != 0": ({"pad_before": ("mod",)}, {}),
    "prev + 1 float": ({"prev_lead": 1}, {}), "prev_sh % 4 != 0": ({"prev_pitch_extra": 5}, {}),
    "angle_col0 % 4 != 0": ({"pad_before": ("angle",)}, {}), "dens_col0 % 4 != 0": ({"pad_before": ("dens",)}, {}),
    "mask + 1 float": ({"mask_lead": 1}, {}), "mask_sh % 4 != 0": ({"mask_pitch_extra": 5}, {}),
}


@pytest.mark.parametrize("why", list(UNPATCH_FALLBACKS) + ["lvl_stride % 4 != 0"])
def test_unpatchify_leaves_the_vector_form(why):
    """P = 4 with one alignment condition of the vector form broken at a time: unpatchify_kernel<1> on the same mix."""
    Wp, n_lvl = 9, 3
    if why == "lvl_stride % 4 != 0":
        y, vars = R.unpatch_inputs(["plain", "clamp"], B, n_lvl, HP, Wp, 4, seed=80, lvl_heads=True, lvl_stride_extra=1,
                                   ldy_extra=1)
        assert vars[0]["lvl_stride"] % 4 == 1 and y.shape[1] % 4 == 0
        check_unpatchify(y, vars, n_lvl, Wp, 4, why)
        return
    build, place = UNPATCH_FALLBACKS[why]
    y, vars = R.unpatch_inputs(R.UNPATCH_MIX, B, n_lvl, HP, Wp, 4, seed=80, **build)
    if "ldy_extra" in build:
        assert y.shape[1] % 4 == 1
    check_unpatchify(y, vars, n_lvl, Wp, 4, why, **place)


@pytest.mark.parametrize("P", [4, 3])
def test_unpatchify_level_conditioned_heads(P):
    """lvl_stride = n_heads P P: level c's head outputs sit c lvl_stride columns further, in rows n_lvl lvl_stride wide (a
    call of its own: the other variables' columns do not move with the level)."""
    n_lvl, Wp = 3, 9
    y, vars = R.unpatch_inputs(["plain", "clamp"], B, n_lvl, HP, Wp, P, seed=90, lvl_heads=True)
    assert vars[0]["lvl_stride"] == 2 * P * P
    check_unpatchify(y, vars, n_lvl, Wp, P, ("lvl_stride", P))


# ------------------------------------------------------------------------------------------
# assemble_tokens
# ------------------------------------------------------------------------------------------
def run_assemble(shape, ins, with_t):
    L = lib()
    Bq, Cl, Lp, D = shape
    rows = Bq * Cl * Lp
    dev = [t.to(DEV) for t in ins]
    before = [t.clone() for t in dev]
    out_f = torch.full((rows + 2, D), NAN, device=DEV)
    out_t = torch.full((rows + 2, D), NAN, dtype=torch.bfloat16, device=DEV) if with_t else None
    L.assemble_tokens(*dev, out_f[:rows], None if out_t is None else out_t[:rows], Bq, Cl, Lp, D)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(dev, before))
    assert bool(torch.isnan(out_f[rows:]).all()) and (out_t is None or bool(torch.isnan(out_t[rows:]).all()))
    if with_t:      # the fp32 stream rounded once
        assert same_bits(out_t[:rows], out_f[:rows].to(torch.bfloat16)), shape
    return dev, out_f[:rows]


@pytest.mark.parametrize("with_t", [True, False], ids=["bf16 copy", "fp32 only"])
@pytest.mark.parametrize("shape", R.ASSEMBLE_SHAPES)
def test_assemble_tokens(shape, with_t):
    ins = R.assemble_inputs(*shape)
    _, out = run_assemble(shape, ins, with_t)
    ref, scale = R.assemble_ref(*ins, *shape)
    assert_close(out, ref, scale, torch.zeros(ref.shape, dtype=torch.long), torch.tensor([R.ASSEMBLE_TOL], dtype=torch.float64),
                 ("assemble", shape, with_t), ("sum",))


@pytest.mark.parametrize("with_t", [True, False], ids=["bf16 copy", "fp32 only"])
def test_assemble_tokens_grid_stride_loop(with_t):
    """More 8-feature pieces than 16384 blocks x 256 threads: the last 4096 pieces are a second trip of the grid-stride
    loop.  The fp64 reference is built on the device; the criterion is that of embed_reference.ratios."""
    shape = R.ASSEMBLE_LOOPED
    assert math.prod(shape) // 8 > 16384 * 256
    dev, out = run_assemble(shape, R.assemble_inputs(*shape), with_t)
    ref, scale = R.assemble_ref(*dev, *shape)
    ratio = (out.double() - ref).abs() / (R.ASSEMBLE_TOL * scale)
    worst = float(ratio.max())
    print("MEASURE assemble loop", worst * 2, "u")
    assert worst <= 1.0 and not bool(torch.isnan(out).any()), worst


def test_assemble_tokens_refuses_a_single_level_and_ragged_rows():
    L = lib()
    for Bq, Cl, Lp, D in ((2, 1, 5, 8), (2, 2, 5, 12)):
        ins = [t.to(DEV) for t in R.assemble_inputs(Bq, max(Cl, 2), Lp, D)]
        out = torch.full((Bq * Cl * Lp, D), NAN, device=DEV)
        with pytest.raises(ValueError, match=f"assemble_tokens: D={D} must be a multiple of 8, Cl={Cl} >= 2"):
            L.assemble_tokens(*ins, out, None, Bq, Cl, Lp, D)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
