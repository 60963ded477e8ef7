"""The fp64 references of tests/embed_reference.py against the oracle, the conditions their input builders promise, and
the teeth of those inputs: every planted fault lands at least 100 x the tolerance of the GPU assertion away from the
right result, by the per-element criterion the GPU tests use (embed_reference.ratios).  Runs without a GPU.

What the oracle offers to compare with: unpatchify, the unfold of patch_embed (as tests/test_gpu_ops.py builds it),
_pollution_pre (transform 2), _wave_pre (transforms 3-6) and _wave_post (direction, density, water mask);
wave_batch_transform works on the raw batch before it is normalised and has no counterpart in these kernels.  The
difference prediction and the SO2 cap exist in the oracle only inside forward(), between the decoder and the
un-normalisation, and assemble_tokens only inside encoder_forward(): there is no function to call, so those stand on
the header's formulas alone.
"""
import math

import pytest
import torch

from oracle import aurora_oracle as oracle
from tests import embed_reference as R

TEETH = 100.0
B, T, HP = 2, 2, 3
PATCH_GRIDS = [(9, 4, 3), (17, 3, 3), (37, 10, 1)]            # (Wp, P, n_lvl)
UNPATCH_GRIDS = [(9, 4, 3), (33, 4, 3), (86, 3, 3), (26, 10, 1)]


def worst(wrong, ref, scale, kind, tols):
    return float(R.ratios(wrong, ref, scale, kind, tols).max())


def far(wrong, ref, scale, kind, tols, what=""):
    err = worst(wrong, ref, scale, kind, tols)
    assert err >= TEETH, (what, err)


# ---- the right references equal the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("P,Wp", [(3, 7), (4, 9), (10, 5)])
def test_unpatchify_ref_equals_the_oracle(P, Wp):
    n_lvl, kinds = 3, ["plain", "clamp", "plain"]
    y, vs = R.unpatch_inputs(kinds, B, n_lvl, HP, Wp, P, ldy_extra=0)
    V, PP = len(kinds), P * P
    y_or = y.reshape(B, HP * Wp, n_lvl, V, PP).permute(0, 1, 2, 4, 3).reshape(B, HP * Wp, n_lvl, PP * V)
    want = oracle.unpatchify(y_or.double(), V, HP * P, Wp * P, P)
    mag = want.abs()                       # (the scale is taken before the clamp: a clamp that binds only shrinks the error)
    want[:, 1] = want[:, 1].clamp(min=0)
    for n, (out, scale, _) in enumerate(R.unpatchify_ref(y, vs, B, n_lvl, HP, Wp, P)):
        sc, loc = vs[n]["scale"].double()[:, None, None], vs[n]["loc"].double()[:, None, None]
        assert (out - (want[:, n] * sc + loc)).abs().max().item() <= 1e-12
        assert (scale - (mag[:, n] * sc + loc.abs())).abs().max().item() <= 1e-12


@pytest.mark.parametrize("P,Wp", [(3, 7), (4, 9), (10, 5)])
def test_patchify_ref_equals_the_unfold(P, Wp):
    n_lvl = 3
    vs = R.patch_inputs([0, 1, 1], B, T, n_lvl, HP, Wp, P, static=True)
    vs[0]["x"].nan_to_num_(0.5)
    H, W, V = HP * P, Wp * P, len(vs)
    norm = []
    for v in vs:
        x = v["x"].double()
        x = x[None, None, None].expand(B, T, n_lvl, -1, -1) if x.dim() == 2 else x
        z = (x[..., :H, :] - v["loc"].double()[:, None, None]) * v["inv"].double()[:, None, None]
        norm.append(z.clamp(min=0) if v["transform"] == 1 else z)
    full = torch.stack(norm, dim=2)                                                   # (B, T, V, C, H, W)
    pat = full.reshape(B, T, V, n_lvl, HP, P, Wp, P).permute(3, 0, 4, 6, 2, 1, 5, 7)  # c b hp wp v t i j
    out, scale, kind = R.patchify_ref(vs, B, T, n_lvl, HP, Wp, P)
    assert torch.equal(out, pat.reshape(n_lvl * B * HP * Wp, V * T * P * P))
    assert torch.equal(scale, out.abs()) and bool((kind == R.PK_LINEAR).all())


def test_transforms_equal_the_oracles_hooks():
    g = R.gen(5)
    z = R.uniform(g, -1, 4, 4000)
    z[:3] = torch.tensor([0.0, R.EPS, R.T2_CAP])
    sd = {"surf_feature_combiner.v.weight": torch.tensor([[0.75, -1.25]], dtype=torch.float64),
          "surf_feature_combiner.v.bias": torch.tensor([0.5], dtype=torch.float64)}
    out, _, _ = R.transform_ref(z, 2, 0.75, -1.25, 0.5)
    assert (out - oracle._pollution_pre(sd, "surf", "v", z.clamp(min=0))).abs().max().item() <= 1e-12
    x = R.uniform(g, 0, 360, 4000)
    x[torch.rand(4000, generator=g) < 0.2] = float("nan")
    pre = oracle._wave_pre({"mwd": x, "swh": x})
    for tr, name in ((3, "swh_density"), (4, "swh"), (5, "mwd_sin"), (6, "mwd_cos")):
        assert (R.transform_ref(x, tr)[0] - pre[name]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("P,Wp", [(3, 5), (4, 9)])
def test_wave_heads_equal_the_oracles_post_hook(P, Wp):
    """The header's rule is `density head >= 0`; the oracle's is sigmoid(head) >= 0.5, which in floating point also holds
    for heads in (-1e-16, 0) (fp64; (-6e-8, 0) in fp32) where the sigmoid rounds to 0.5.  The builders' -1e-30 is such a
    head: it is moved to -0.5 here, everything else (0.0, -0.0, +1e-30, the mask ties) is compared as built."""
    n_lvl = 1
    y, vs = R.unpatch_inputs(["dir_dens", "val_dens"], B, n_lvl, HP, Wp, P)
    y[y == -1e-30] = -0.5
    H, W = HP * P, Wp * P

    def field(col0):   # head block -> (B, H, W), plain
        v = dict(vs[1], col0=col0, dens_col0=-1, loc=torch.zeros(1), scale=torch.ones(1))
        return R.unpatchify_ref(y, [v], B, n_lvl, HP, Wp, P)[0][0][:, 0]

    d, s = vs[0], vs[1]
    pred = {"mwd_sin": field(d["col0"]), "mwd_cos": field(d["angle_col0"]), "mwd_density": field(d["dens_col0"]),
            "swh": field(s["col0"]), "swh_density": field(s["dens_col0"])}
    for v in (d, s):   # the builder gives both variables a mask of their own
        wmb = v["mask"].double()[v["mask_off"]:].reshape(H, v["mask_sh"])[:, :W] - v["mask_thresh"]
        post = oracle._wave_post(dict(pred), wmb)
        out = R.unpatchify_ref(y, [v], B, n_lvl, HP, Wp, P)[0][0][:, 0]
        want = post["mwd" if v is d else "swh"] * v["scale"].double()[0] + v["loc"].double()[0]
        assert torch.equal(torch.isnan(out), torch.isnan(want)) and 0.1 < float(torch.isnan(out).double().mean()) < 0.9
        assert (out - want).nan_to_num(0.0).abs().max().item() <= 1e-10


# ---- the builders keep their promises -----------------------------------------------------------------------
@pytest.mark.parametrize("Wp,P,n_lvl", UNPATCH_GRIDS)
def test_unpatch_builder_conditions(Wp, P, n_lvl):
    y, vs = R.unpatch_inputs(R.UNPATCH_MIX, B, n_lvl, HP, Wp, P)
    by = {v["kind"]: v for v in vs}
    cap, clamp = R.binding_fractions(y, by["diff_cap_clamp"], B, n_lvl, HP, Wp, P)
    assert 0.2 < cap < 0.5 and 0.2 < clamp < 0.5, (cap, clamp)
    for k in ("dir", "dir_dens"):
        v = dict(by[k], dens_col0=-1, loc=torch.zeros(n_lvl), scale=torch.ones(n_lvl))
        deg = R.unpatchify_ref(y, [v], B, n_lvl, HP, Wp, P)[0][0]
        rest = deg.clone()
        for n, (_, _, want) in enumerate(R.EXACT_DIRECTIONS):   # head row 0 = (b, patch, level) 0: in-patch pixels 0 .. 4
            assert deg[0, 0, n // P, n % P].item() == want
            rest[0, 0, n // P, n % P] = 180.0
        assert bool(((rest >= R.ANGLE_MARGIN) & (rest <= 360 - R.ANGLE_MARGIN)).all())
    for k in ("dir_dens", "val_dens"):
        v = by[k]
        dens = y[:, v["dens_col0"]:v["dens_col0"] + P * P]
        for val in (1e-30, -1e-30):
            assert bool((dens == val).any())
        zeros = dens[dens == 0]
        assert bool(torch.signbit(zeros).any()) and bool((~torch.signbit(zeros)).any())
        m = v["mask"][v["mask_off"]:]
        assert bool((m == v["mask_thresh"]).any() and (m > v["mask_thresh"]).any() and (m < v["mask_thresh"]).any())


def test_patch_builder_conditions():
    vs = R.patch_inputs(R.patch_transforms(7), B, T, 3, HP, 9, 4)
    assert int(torch.isnan(vs[0]["x"]).sum()) == 3
    v = vs[2]
    z = (v["x"].double() - v["loc"].double()[:, None, None]) * v["inv"].double()[:, None, None]
    assert z[0, 0, 0, 0, :3].tolist() == [0.0, float(torch.tensor(R.EPS).float()), R.T2_CAP]
    for lo, hi in ((-math.inf, 0.0), (0.0, R.EPS), (R.EPS, R.T2_CAP), (R.T2_CAP, math.inf)):
        assert 0.15 < float(((z > lo) & (z < hi)).double().mean()) < 0.35
    for v in vs[3:]:
        assert 0.1 < float(torch.isnan(v["x"]).double().mean()) < 0.3
    for v in vs[5:]:
        z = (v["x"].double() - v["loc"].double()[:, None, None]) * v["inv"].double()[:, None, None]
        assert bool(((z >= 0) & (z < 360) | torch.isnan(z)).all())


# ---- the planted faults are far away on the GPU tests' inputs -----------------------------------------------
@pytest.mark.parametrize("Wp,P,n_lvl", PATCH_GRIDS)
def test_patchify_planted_faults(Wp, P, n_lvl):
    vs = R.patch_inputs(R.patch_transforms(7), B, T, n_lvl, HP, Wp, P, static=True)
    args = (vs, B, T, n_lvl, HP, Wp, P)
    ref, scale, kind = R.patchify_ref(*args)
    faults = {"col_order_tv": {"col_order_tv": True}, "ij_swapped": {"ij_swapped": True},
              "t2_no_clamp": {"t2_no_clamp": True}, "t2_log_eps_sign": {"t2_log_eps_sign": True}}
    if n_lvl > 1:
        faults["rows_batch_level"] = {"rows_batch_level": True}
    for v in range(1, 7):
        faults[f"identity {v}"] = {"identity": v}
    for name, kw in faults.items():
        far(R.patchify_ref(*args, **kw)[0], ref, scale, kind, R.PATCH_TOL, name)
    far(R.mutate_shift_last_patch(ref, B, n_lvl, HP, Wp), ref, scale, kind, R.PATCH_TOL, "shifted patch")
    # padding not zeroed: the padding columns are held to exact zeros (scale 0), whatever else they hold is infinitely far
    pad = torch.zeros(ref.shape[0], 5, dtype=torch.float64)
    zeros, exact = torch.zeros_like(pad), torch.full(pad.shape, R.PK_EXACT, dtype=torch.long)
    for left in (float("nan"), 1e-30):
        assert worst(pad + left, zeros, zeros, exact, R.PATCH_TOL) == math.inf


@pytest.mark.parametrize("Wp,P,n_lvl", UNPATCH_GRIDS)
def test_unpatchify_planted_faults(Wp, P, n_lvl):
    y, vs = R.unpatch_inputs(R.UNPATCH_MIX, B, n_lvl, HP, Wp, P)
    args = (y, vs, B, n_lvl, HP, Wp, P)
    ref = R.unpatchify_ref(*args)
    by = {v["kind"]: n for n, v in enumerate(vs)}

    def check(fault, kinds):
        wrong = R.unpatchify_ref(*args, **{fault: True})
        for k in kinds:
            far(wrong[by[k]][0], *ref[by[k]], R.UNPATCH_TOL, (fault, k))

    check("prev_sh_is_w", ["diff_surf"])
    check("ignore_prev_sb", ["diff_surf", "diff_atm", "diff_cap_clamp"])
    check("inv_is_scale", ["diff_surf", "diff_atm", "diff_cap_clamp"])
    check("cap_before_diff", ["diff_cap_clamp"])
    check("cap_bit_shift", ["diff_cap_clamp"])   # (levels 0b101: level c reads bit c + 1, so the cap moves to level 1 or is lost)
    check("sincos_swapped", ["dir", "dir_dens"])
    check("no_plus_360", ["dir", "dir_dens"])
    check("dens_gt0", ["dir_dens", "val_dens"])
    check("mask_ge", ["dir_dens", "val_dens"])
    check("mask_sh_is_p", ["dir_dens", "val_dens"])


@pytest.mark.parametrize("Wp,P,n_lvl", [(9, 4, 3), (7, 3, 3)])
def test_lvl_stride_planted_fault(Wp, P, n_lvl):
    y, vs = R.unpatch_inputs(["plain", "clamp"], B, n_lvl, HP, Wp, P, lvl_heads=True)
    assert all(v["lvl_stride"] == 2 * P * P for v in vs) and y.shape[1] >= n_lvl * 2 * P * P
    ref = R.unpatchify_ref(y, vs, B, n_lvl, HP, Wp, P)
    wrong = R.unpatchify_ref(y, vs, B, n_lvl, HP, Wp, P, ignore_lvl_stride=True)
    for (w, _, _), (r, s, k) in zip(wrong, ref):
        far(w, r, s, k, R.UNPATCH_TOL, "ignore_lvl_stride")


@pytest.mark.parametrize("shape", R.ASSEMBLE_SHAPES)
def test_assemble_planted_faults(shape):
    ins = R.assemble_inputs(*shape)
    ref, scale = R.assemble_ref(*ins, *shape)
    kind, tols = torch.zeros(ref.shape, dtype=torch.long), torch.tensor([R.ASSEMBLE_TOL], dtype=torch.float64)
    for fault in ("c_off_by_one", "pos_by_blc"):
        far(R.assemble_ref(*ins, *shape, **{fault: True})[0], ref, scale, kind, tols, fault)
    # the reference itself, spelled out token by token
    Bq, Cl, L, D = shape
    surf, agg, pos, te = (t.double() for t in ins)
    for b, c, l in ((0, 0, 0), (Bq - 1, Cl - 1, L - 1), (Bq - 1, 1, L // 2)):
        src = surf[b * L + l] if c == 0 else agg[(b * L + l) * (Cl - 1) + c - 1]
        assert torch.equal(ref[(b * Cl + c) * L + l], src + pos[l] + te[b])
