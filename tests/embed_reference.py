"""fp64 definitions of patchify, unpatchify and assemble_tokens (csrc/embed.hip), the inputs their GPU tests use, and
wrong variants.

Plain torch on the CPU, written from the formulas of include/aurora_hip.h (aurora_patch_var, aurora_unpatch_var,
aurora_hip_assemble_tokens) and not from the kernels or from oracle/ (tests/test_embed_reference.py cross-checks the
latter).  Every reference returns, next to the fp64 result, a per-element SCALE -- the size of the terms an fp32
evaluation has to round -- and a per-element KIND that selects the tolerance.  Results are judged element by element,
|out - ref| <= TOL[kind] * scale, no element excluded, NaN positions equal (`ratios`).

Tolerances.  u = 2^-24 is the unit roundoff of fp32; a rounding has relative error <= u / (1 + u), so k roundings of a
product chain stay strictly below k u and the bounds below need no second-order slack.

patchify (kind = PK_*; the reference is given the fp32 loc and inv_scale the kernel is given):
  PK_LINEAR  transforms 0, 1, 4: z = fl(fl(x - loc) inv), two roundings, clamp and nan_to_num exact.  scale |result|,
             tolerance 2 u.
  PK_EXACT   transform 3: 0 or 1, and every NaN -> 0 of transforms 4-6.  scale 0: equality.
  PK_T2      transform 2: tw0 f0 + tw1 f1 + tb with f0 = min(max(z, 0), 2.5) (2 u relative, from z) and
             f1 = (log(max(z, 1e-4)) - log 1e-4) / -log 1e-4.  scale |tw0 f0| + |tw1 f1| + |tb|.  Counted: z 2, the two
             constants 1e-4f and fl(log 1e-4) 2, the subtraction 1, the division 1, two products and two sums 4 -- ten
             roundings before logf's own error, which this project does not record and for which no HIP math
             documentation was at hand: the constant is MEASURED (below).
  PK_TRIG    transforms 5, 6: sinf / cosf of x_rad = fl(z fl(pi/180)); the argument carries four roundings (z 2, the
             constant, the product), i.e. <= 4 u |x_rad|, which a 1-Lipschitz function passes on, plus the function's
             own error at scale 1.  scale |x_rad| + 1; the constant is MEASURED.
unpatchify (kind = UK_*; scale = (sum of the magnitudes of the terms added) |scale_v| + |loc_v|):
  UK_PLAIN   fl(fl(z scale) + loc): 2 u (|z scale| + |loc|).  The clamps, the density and mask decisions are exact.
  UK_DIFF    z = y + (1 + mod) ((prev - loc) inv): prev term 2 roundings, 1 + mod 1, product 1 -> 4 u |(1 + mod) p|, the
             sum 1 on |y| + |(1 + mod) p|, then the 2 of UK_PLAIN: 7 u ((|y| + |(1 + mod) p|) |scale| + |loc|).  min and
             max are 1-Lipschitz: a clamp that binds only shrinks the error.
  UK_ANGLE   rad2deg(atan2f(sin, cos)) mod 360: scale 360 |scale| + |loc| (absolute error against the full circle).
             atan2f's own error is not recorded; MEASURED.
assemble    fl(fl(a + b) + c): 2 u (|a| + |b| + |c|).

MEASURED constants: worst element error over these inputs against THIS fp64 reference on an MI355X (never against
another kernel form), times 4, capped at 16 u of the scale.  The measured worst value stands next to each constant.
The same run showed what the DERIVED bounds leave: PK_LINEAR 1.99 u of 2, UK_PLAIN 1.00 u of 2, UK_DIFF 3.24 u of 7,
assemble 1.95 u of 2.

The keyword-only arguments of the references, and the `mutate_*` helpers, are deliberately WRONG evaluations, each a
mistake a kernel could plausibly make.  The GPU tests never use them; tests/test_embed_reference.py shows that on the
inputs below each lands at least 100 x the tolerance away from the right result.
"""
import math

import torch

U = 2.0 ** -24

PK_LINEAR, PK_EXACT, PK_T2, PK_TRIG = 0, 1, 2, 3
T2_MEASURED = 6.31 * U     # worst |out - ref| / scale of the transform-2 elements over all patchify cases of test_gpu_embed.py
                           # (4 x = 25 u: the 16 u cap is what holds)
TRIG_MEASURED = 2.13 * U   # the same for transforms 5 and 6: tolerance 8.5 u
PATCH_TOL = torch.tensor([2 * U, 0.0, min(4 * T2_MEASURED, 16 * U), min(4 * TRIG_MEASURED, 16 * U)], dtype=torch.float64)

UK_PLAIN, UK_DIFF, UK_ANGLE = 0, 1, 2
ANGLE_MEASURED = 1.78 * U  # worst |out - ref| / (360 |scale| + |loc|) of the direction variables over all unpatchify cases:
                           # tolerance 7.1 u
UNPATCH_TOL = torch.tensor([2 * U, 7 * U, min(4 * ANGLE_MEASURED, 16 * U)], dtype=torch.float64)

ASSEMBLE_TOL = 2 * U

EPS = 1e-4
T2_CAP = 2.5
MASK_THRESH = 0.25
ANGLE_MARGIN = 1.0          # degrees kept from the 0 / 360 wrap by the direction builders
# (sin, cos) heads with an exactly known direction; they sit at the first in-patch pixels of the first head row
EXACT_DIRECTIONS = [(0.0, 1.0, 0.0), (0.0, -1.0, 180.0), (-1.0, 0.0, 270.0), (1.0, 0.0, 90.0), (-0.0, 1.0, 0.0)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def uniform(g, lo, hi, *shape):
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------------------------------
# the criterion
# ------------------------------------------------------------------------------------------
def ratios(out, ref, scale, kind, tols):
    """Per element |out - ref| / (tols[kind] * scale) in fp64 on the CPU: <= 1 passes.  0 where both are NaN or equal;
    inf where exactly one is NaN or where a difference meets a zero tolerance."""
    out, ref = out.detach().double().cpu(), ref.double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    tol = tols[kind] * scale
    diff = (out - ref).abs()
    r = diff / tol
    r = torch.where(diff == 0, torch.zeros_like(r), r)
    both, one = torch.isnan(out) & torch.isnan(ref), torch.isnan(out) ^ torch.isnan(ref)
    r = torch.where(both, torch.zeros_like(r), r)
    return torch.where(one | torch.isnan(r), torch.full_like(r, math.inf), r)


def worst_by_kind(out, ref, scale, kind, n_kinds):
    """max |out - ref| / scale per kind in units of u (what the MEASURED constants record); 0 for an absent kind."""
    r = ratios(out, ref, scale, kind, torch.full((n_kinds,), U, dtype=torch.float64))
    return [float(r[kind == k].max()) if bool((kind == k).any()) else 0.0 for k in range(n_kinds)]


# ------------------------------------------------------------------------------------------
# patchify
# ------------------------------------------------------------------------------------------
def transform_ref(z, tr, tw0=0.0, tw1=0.0, tb=0.0, *, t2_no_clamp=False, t2_log_eps_sign=False):
    """f_v of aurora_patch_var on fp64 z: (result, scale, kind)."""
    zero = torch.zeros_like(z)
    kind = torch.full(z.shape, PK_LINEAR, dtype=torch.long)
    if tr == 0:
        return z, z.abs().nan_to_num(0.0), kind
    if tr == 1:
        r = z.clamp(min=0)
        return r, r.abs(), kind
    if tr == 2:
        zc = z if t2_no_clamp else z.clamp(min=0)
        f0 = zc.clamp(max=T2_CAP)
        log_eps = -math.log(EPS) if t2_log_eps_sign else math.log(EPS)
        f1 = (torch.log(zc.clamp(min=EPS)) - log_eps) / (-log_eps)
        return tw0 * f0 + tw1 * f1 + tb, (tw0 * f0).abs() + (tw1 * f1).abs() + abs(tb), kind.fill_(PK_T2)
    nan = torch.isnan(z)
    if tr == 3:
        return (~nan).double(), zero, kind.fill_(PK_EXACT)
    if tr == 4:
        r = torch.where(nan, zero, z)
        kind[nan] = PK_EXACT
        return r, r.abs(), kind
    if tr in (5, 6):
        rad = z * (math.pi / 180.0)
        r = torch.where(nan, zero, torch.sin(rad) if tr == 5 else torch.cos(rad))
        kind.fill_(PK_TRIG)
        kind[nan] = PK_EXACT
        return r, torch.where(nan, zero, rad.abs() + 1.0), kind
    raise ValueError(tr)


def patchify_ref(vars, B, T, n_lvl, Hp, Wp, P, *, col_order_tv=False, ij_swapped=False, rows_batch_level=False,
                 identity=None, t2_no_clamp=False, t2_log_eps_sign=False):
    """The GEMM operand (n_lvl B Hp Wp, K) of aurora_hip_patchify in fp64, rows (level, batch, hp, wp), columns
    (v, t, i, j): (operand, scale, kind).  `vars`: dicts with x (B, T, n_lvl, >= H, >= W) or a static plane (>= H, >= W),
    fp32 loc and inv (n_lvl), transform, tw0, tw1, tb.
    WRONG `col_order_tv`: columns (t, v, i, j).  WRONG `ij_swapped`: (v, t, j, i).  WRONG `rows_batch_level`: rows
    (batch, level, hp, wp).  WRONG `identity` = v: variable v's transform left out.  WRONG `t2_no_clamp`: transform 2
    without its clamp at 0.  WRONG `t2_log_eps_sign`: log eps taken as +9.21."""
    H, W, V = Hp * P, Wp * P, len(vars)
    parts = []
    for n, v in enumerate(vars):
        x = v["x"].double()
        if x.dim() == 2:
            x = x[None, None, None].expand(B, T, n_lvl, -1, -1)
        z = (x[..., :H, :W] - v["loc"].double()[:, None, None]) * v["inv"].double()[:, None, None]
        parts.append(transform_ref(z, 0 if identity == n else v["transform"], v["tw0"], v["tw1"], v["tb"],
                                   t2_no_clamp=t2_no_clamp, t2_log_eps_sign=t2_log_eps_sign))

    def operand(a):   # (V, B, T, C, H, W) -> rows x K
        a = a.reshape(V, B, T, n_lvl, Hp, P, Wp, P)          # v0 b1 t2 c3 hp4 i5 wp6 j7
        rows = (1, 3) if rows_batch_level else (3, 1)
        vt = (2, 0) if col_order_tv else (0, 2)
        ij = (7, 5) if ij_swapped else (5, 7)
        return a.permute(*rows, 4, 6, *vt, *ij).reshape(n_lvl * B * Hp * Wp, V * T * P * P)

    return tuple(operand(torch.stack([p[k] for p in parts])) for k in range(3))


def mutate_shift_last_patch(op, B, n_lvl, Hp, Wp):
    """WRONG: the last patch of every patch row holds its left neighbour's values (a ragged last group walked one short)."""
    o = op.clone().reshape(n_lvl * B * Hp, Wp, -1)
    o[:, Wp - 1] = o[:, Wp - 2]
    return o.reshape(op.shape)


def patch_transforms(n):
    """n transform codes: every code 0-6 in turn."""
    return [k % 7 for k in range(n)]


def patch_inputs(transforms, B, T, n_lvl, Hp, Wp, P, static=False, seed=0):
    """One variable per entry of `transforms` (+ a static transform-0 plane if `static`), each with one latitude row
    more than the patches cover.  Values are chosen per transform in NORMALISED units z and mapped back to raw
    x = z / inv + loc in fp32; the references take those fp32 values.
      0: z in +-3; the first such variable carries three NaN.         1: z in +-3 (half of them clamped).
      2: a quarter each below 0, in (0, 1e-4), in (1e-4, 2.5) log-uniformly, above 2.5; level 0 has loc 0, inv 1 and
         the exact values 0, 1e-4f and 2.5 in its first three pixels; inv is a power of two at every level.
      3, 4: z in +-3 with ~20 % NaN.         5, 6: degrees in [0, 360) with ~20 % NaN (asserted)."""
    g = gen(1000 + seed)
    H, W = Hp * P, Wp * P
    shape = (B, T, n_lvl, H + 1, W)
    out, seen0 = [], False
    for tr in transforms:
        loc = uniform(g, -1, 1, n_lvl).float()
        inv = (1.0 / uniform(g, 0.5, 1.5, n_lvl)).float()
        tw0 = tw1 = tb = 0.0
        if tr == 2:
            z = uniform(g, 0, 1, *shape)
            cls = torch.randint(0, 4, shape, generator=g)
            lo, hi = math.log(EPS * 1.01), math.log(T2_CAP * 0.99)
            z = torch.where(cls == 0, -3 * z - 1e-3,
                            torch.where(cls == 1, EPS * (0.01 + 0.98 * z),
                                        torch.where(cls == 2, torch.exp(lo + (hi - lo) * z), T2_CAP + 0.01 + 3.5 * z)))
            inv = torch.tensor([1.0, 2.0, 0.5, 4.0])[torch.arange(n_lvl) % 4]
            loc[0] = 0.0
            tw0, tw1, tb = 0.75, -1.25, 0.5
        elif tr in (5, 6):
            z = uniform(g, 0.5, 359.5, *shape)
        else:
            z = uniform(g, -3, 3, *shape)
        x = (z / inv.double()[:, None, None] + loc.double()[:, None, None]).float()
        if tr == 2:
            x[0, 0, 0, 0, :3] = torch.tensor([0.0, EPS, T2_CAP])   # (EPS rounds to the kernel's 1e-4f)
        if tr >= 3:
            x[torch.rand(shape, generator=g) < 0.2] = float("nan")
        if tr in (5, 6):
            zz = (x.double() - loc.double()[:, None, None]) * inv.double()[:, None, None]
            assert bool(((zz >= 0) & (zz < 360) | torch.isnan(zz)).all())
        if tr == 0 and not seen0:
            seen0 = True
            x.view(-1)[torch.tensor([0, x.numel() // 2, x.numel() - W - 1])] = float("nan")
        out.append({"x": x, "loc": loc, "inv": inv, "transform": tr, "tw0": tw0, "tw1": tw1, "tb": tb})
    if static:
        out.append({"x": uniform(g, -2, 2, H + 1, W).float(), "loc": uniform(g, -1, 1, n_lvl).float(),
                    "inv": (1.0 / uniform(g, 0.5, 1.5, n_lvl)).float(), "transform": 0, "tw0": 0.0, "tw1": 0.0, "tb": 0.0})
    return out


# ------------------------------------------------------------------------------------------
# unpatchify
# ------------------------------------------------------------------------------------------
def _gather(buf, idx):
    return buf.double()[idx.clamp(0, buf.numel() - 1)]


def unpatchify_ref(y, vars, B, n_lvl, Hp, Wp, P, *, prev_sh_is_w=False, ignore_prev_sb=False, inv_is_scale=False,
                   cap_before_diff=False, cap_bit_shift=False, sincos_swapped=False, no_plus_360=False, dens_gt0=False,
                   mask_ge=False, mask_sh_is_p=False, ignore_lvl_stride=False):
    """dst_v[b][c][h][w] of aurora_hip_unpatchify in fp64 for every variable: a list of (dst, scale, kind).  `y`: fp32
    (B Hp Wp n_lvl, ldy); `vars`: dicts with the members of aurora_unpatch_var, the planes `prev` and `mask` as flat fp32
    buffers plus the offset of their first element (prev_off, mask_off).  Hooks in the header's order: difference
    prediction, min(z, 1) on the flagged levels, max(z, 0), atan2 -> degrees -> mod 360, density / mask -> NaN,
    z scale + loc.
    WRONG variants: `prev_sh_is_w` (rows of prev taken W apart), `ignore_prev_sb` (batch 0's prev for every b),
    `inv_is_scale`, `cap_before_diff` (min(y, 1) before the difference is added -- the cap in the wrong place that can
    be seen: min(., 1) and max(., 0) commute, so a cap applied AFTER the clamp gives the same field and is no fault to
    plant), `cap_bit_shift` (level c tests bit c + 1), `sincos_swapped`, `no_plus_360`, `dens_gt0` (density > 0 instead of >= 0), `mask_ge` (mask >= threshold),
    `mask_sh_is_p` (mask rows inside a patch taken P apart), `ignore_lvl_stride`."""
    H, W, L = Hp * P, Wp * P, Hp * Wp
    yd = y.double()
    b, c, h, w = torch.meshgrid(torch.arange(B), torch.arange(n_lvl), torch.arange(H), torch.arange(W), indexing="ij")
    row = (b * L + (h // P) * Wp + w // P) * n_lvl + c
    results = []
    for v in vars:
        base = (0 if ignore_lvl_stride else c * v["lvl_stride"]) + (h % P) * P + w % P
        loc, sc = v["loc"].double()[c], v["scale"].double()[c]
        z = yd[row, base + v["col0"]]
        mag = z.abs()
        kind = torch.full(z.shape, UK_PLAIN, dtype=torch.long)
        cap = ((v["cap_levels"] >> (c + 1 if cap_bit_shift else c)) & 1).bool()
        if v["mod_col0"] >= 0:
            idx = (v["prev_off"] + (0 if ignore_prev_sb else b * v["prev_sb"]) + c * v["prev_sc"]
                   + h * (W if prev_sh_is_w else v["prev_sh"]) + w)
            inv = sc if inv_is_scale else v["inv"].double()[c]
            term = (1.0 + yd[row, base + v["mod_col0"]]) * ((_gather(v["prev"], idx) - loc) * inv)
            if cap_before_diff:
                z = torch.where(cap, z.clamp(max=1.0), z)
            z, mag = z + term, mag + term.abs()
            kind.fill_(UK_DIFF)
        if not cap_before_diff:
            z = torch.where(cap, z.clamp(max=1.0), z)
        if v["clamp_min0"]:
            z = z.clamp(min=0.0)
        if v["angle_col0"] >= 0:
            s, co = z, yd[row, base + v["angle_col0"]]
            z = torch.rad2deg(torch.atan2(co, s) if sincos_swapped else torch.atan2(s, co))
            z = torch.fmod(z, 360.0)
            if not no_plus_360:
                z = torch.where(z < 0, z + 360.0, z)
            mag = torch.full_like(z, 360.0)
            kind.fill_(UK_ANGLE)
        if v["dens_col0"] >= 0:
            dens = yd[row, base + v["dens_col0"]]
            if mask_sh_is_p:
                midx = v["mask_off"] + (h // P) * P * v["mask_sh"] + (h % P) * P + w
            else:
                midx = v["mask_off"] + h * v["mask_sh"] + w
            m = _gather(v["mask"], midx)
            water = (m >= v["mask_thresh"]) if mask_ge else (m > v["mask_thresh"])
            keep = water & ((dens > 0) if dens_gt0 else (dens >= 0))
            z = torch.where(keep, z, torch.full_like(z, float("nan")))
        results.append((z * sc + loc, mag * sc.abs() + loc.abs(), kind))
    return results


UNPATCH_MIX = ["plain", "clamp", "diff_surf", "diff_atm", "diff_cap_clamp", "dir", "dir_dens", "val_dens"]


def unpatch_inputs(kinds, B, n_lvl, Hp, Wp, P, seed=0, *, pad_before=(), ldy_extra=4, prev_lead=0, mask_lead=0,
                   prev_pitch_extra=4, mask_pitch_extra=4, lvl_heads=False, lvl_stride_extra=0):
    """(y, vars) for one unpatchify call with one variable per entry of `kinds`:
      plain | clamp (y in -1 .. 2: a third clamped) |
      diff_surf (prev one plane per batch element, prev_sc = 0, rows W + prev_pitch_extra apart) |
      diff_atm (prev = history step 1 of a (B, 2, n_lvl, H, W) array: prev_sb = 2 n_lvl H W, prev_sc = H W) |
      diff_cap_clamp (diff_atm + min(z, 1) on levels 0b101 + max(z, 0)) | dir (scale 1, loc 0) |
      dir_dens (direction + density + mask, mask rows W + mask_pitch_extra apart) | val_dens (value + density + mask).
    Difference variables have y in +-0.3, mod in +-0.2 and a normalised prev in -1 .. 2, so that z is below 0, inside
    (0, 1) and above 1 on about a third of the elements each.  Directions: radius 0.5 .. 1.5, angle at least ANGLE_MARGIN
    degrees from the wrap (asserted on the fp32 heads), and EXACT_DIRECTIONS in the first pixels of head row 0.  Density
    heads in +-1 with 0.0, -0.0 and +-1e-30 among them; mask values around MASK_THRESH with exact ties.
    Head columns are laid out one P x P block after another; a block named in `pad_before` ("col0", "mod", "angle",
    "dens") starts one column late (and the next one is re-aligned).  `lvl_heads`: level-conditioned heads, every variable
    with lvl_stride = len(kinds) P P + lvl_stride_extra and rows n_lvl lvl_stride wide."""
    g = gen(2000 + seed)
    H, W, PP, L = Hp * P, Wp * P, P * P, Hp * Wp
    rows = B * L * n_lvl
    cur, blocks = 0, []

    def block(name, values):
        nonlocal cur
        cur += 1 if name in pad_before else 0
        blocks.append((cur, values))
        cur += PP + (3 if name in pad_before else 0)
        return blocks[-1][0]

    vars = []
    for k in kinds:
        loc, scale = uniform(g, -1, 1, n_lvl).float(), uniform(g, 0.5, 1.5, n_lvl).float()
        if k == "dir":
            loc, scale = torch.zeros(n_lvl), torch.ones(n_lvl)
        v = {"kind": k, "loc": loc, "scale": scale, "inv": (1.0 / scale.double()).float(), "clamp_min0": 0, "lvl_stride": 0,
             "mod_col0": -1, "prev": None, "prev_off": 0, "prev_sb": 0, "prev_sc": 0, "prev_sh": 0, "cap_levels": 0,
             "angle_col0": -1, "dens_col0": -1, "mask": None, "mask_off": 0, "mask_sh": 0, "mask_thresh": MASK_THRESH}
        if k in ("plain", "val_dens"):
            v["col0"] = block("col0", uniform(g, -2, 2, rows, PP))
        elif k == "clamp":
            v["col0"] = block("col0", uniform(g, -1, 2, rows, PP))
            v["clamp_min0"] = 1
        elif k.startswith("diff"):
            v["col0"] = block("col0", uniform(g, -0.3, 0.3, rows, PP))
            v["mod_col0"] = block("mod", uniform(g, -0.2, 0.2, rows, PP))
            if k == "diff_surf":
                pitch = W + prev_pitch_extra
                pn = uniform(g, -1, 2, B, 1, H, pitch)
                v.update(prev_sb=H * pitch, prev_sc=0, prev_sh=pitch)
                raw = pn * scale.double()[0] + loc.double()[0]   # (one plane serves every level: a surface variable)
            else:
                pn = uniform(g, -1, 2, B, 2, n_lvl, H, W)
                v.update(prev_sb=2 * n_lvl * H * W, prev_sc=H * W, prev_sh=W, prev_off=n_lvl * H * W)
                raw = pn * scale.double()[:, None, None] + loc.double()[:, None, None]
            v["prev_off"] += prev_lead
            v["prev"] = torch.cat([torch.zeros(prev_lead, dtype=torch.float64), raw.reshape(-1)]).float()
            if k == "diff_cap_clamp":
                v.update(cap_levels=0b101, clamp_min0=1)
        elif k in ("dir", "dir_dens"):
            theta = torch.deg2rad(uniform(g, 2 * ANGLE_MARGIN, 360 - 2 * ANGLE_MARGIN, rows, PP))
            r = uniform(g, 0.5, 1.5, rows, PP)
            s, co = (r * torch.sin(theta)).float(), (r * torch.cos(theta)).float()
            deg = torch.rad2deg(torch.atan2(s.double(), co.double())) % 360
            assert bool(((deg >= ANGLE_MARGIN) & (deg <= 360 - ANGLE_MARGIN)).all())
            for n, (es, ec, _) in enumerate(EXACT_DIRECTIONS):
                s[0, n], co[0, n] = es, ec
            v["col0"] = block("col0", s)
            v["angle_col0"] = block("angle", co)
        else:
            raise ValueError(k)
        if k in ("dir_dens", "val_dens"):
            dens = uniform(g, -1, 1, rows, PP).float()
            for val in (0.0, -0.0, 1e-30, -1e-30):      # ~2 % each: some of them always lie over water
                dens[torch.rand(rows, PP, generator=g) < 0.02] = val
            dens[1, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
            dens[rows - 1, PP - 4:] = torch.tensor([-1e-30, 1e-30, -0.0, 0.0])
            v["dens_col0"] = block("dens", dens)
            pitch = W + mask_pitch_extra
            m = (MASK_THRESH + uniform(g, -1, 1, H, pitch)).float()
            m[torch.rand(H, pitch, generator=g) < 0.1] = MASK_THRESH
            v.update(mask=torch.cat([torch.zeros(mask_lead), m.reshape(-1)]), mask_off=mask_lead, mask_sh=pitch)
        vars.append(v)
    if lvl_heads:
        assert all(k in ("plain", "clamp") for k in kinds)
        stride = cur + lvl_stride_extra
        y = uniform(g, -1, 2, rows, n_lvl * stride + ldy_extra).float()   # every level's columns differ
        for v in vars:
            v["lvl_stride"] = stride
        return y, vars
    y = uniform(g, -1, 1, rows, cur + ldy_extra).float()
    for col, values in blocks:
        y[:, col:col + PP] = values.float()
    return y, vars


def binding_fractions(y, v, B, n_lvl, Hp, Wp, P):
    """(fraction of the flagged-level elements where min(z, 1) binds, fraction of all elements where max(z, 0) binds) of a
    difference variable."""
    free = dict(v, cap_levels=0, clamp_min0=0)
    z = (unpatchify_ref(y, [free], B, n_lvl, Hp, Wp, P)[0][0] - v["loc"].double()[None, :, None, None]) \
        / v["scale"].double()[None, :, None, None]
    flagged = torch.tensor([(v["cap_levels"] >> c) & 1 for c in range(n_lvl)]).bool()
    capped = torch.where(flagged[None, :, None, None], z.clamp(max=1.0), z)
    return float((z[:, flagged] > 1).double().mean()) if bool(flagged.any()) else 0.0, float((capped < 0).double().mean())


# ------------------------------------------------------------------------------------------
# assemble_tokens
# ------------------------------------------------------------------------------------------
def assemble_ref(surf, agg, pos_scale, time_emb, B, Cl, L, D, *, c_off_by_one=False, pos_by_blc=False):
    """x[b][c][l] = (c == 0 ? surf[b][l] : agg[(b L + l)(Cl - 1) + c - 1]) + pos_scale[l] + time_emb[b] in fp64, on the
    device of the inputs: ((B Cl L, D), scale), scale = |a| + |b| + |c|.
    WRONG `c_off_by_one`: latent level c reads agg's level c (clamped to the rows there are) instead of c - 1.
    WRONG `pos_by_blc`: pos_scale indexed as if the tokens were laid out (b, l, c)."""
    a = agg.double().reshape(B * L * (Cl - 1), D)
    if c_off_by_one:
        a = a[(torch.arange(a.shape[0], device=a.device) + 1).clamp(max=a.shape[0] - 1)]
    x = torch.cat([surf.double().reshape(B, 1, L, D), a.reshape(B, L, Cl - 1, D).permute(0, 2, 1, 3)], dim=1)
    pos = pos_scale.double()
    if pos_by_blc:
        tok = torch.arange(B * Cl * L, device=pos.device)
        pos = pos[(tok // Cl) % L].reshape(B, Cl, L, D)
    else:
        pos = pos[None, None].expand(B, Cl, L, D)
    te = time_emb.double()[:, None, None].expand(B, Cl, L, D)
    return (x + pos + te).reshape(-1, D), (x.abs() + pos.abs() + te.abs()).reshape(-1, D)


def assemble_inputs(B, Cl, L, D, seed=0):
    g = gen(3000 + seed)
    return (uniform(g, -1, 1, B * L, D).float(), uniform(g, -1, 1, B * L * (Cl - 1), D).float(),
            uniform(g, -1, 1, L, D).float(), uniform(g, -1, 1, B, D).float())


ASSEMBLE_SHAPES = [(2, 2, 5, 8), (2, 4, 30, 64), (1, 3, 7, 4096)]
ASSEMBLE_LOOPED = (1, 2, 4100, 4096)    # B Cl L D / 8 = 4 198 400 pieces > 16384 blocks x 256 threads = 4 194 304
