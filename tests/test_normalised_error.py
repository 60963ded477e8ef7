"""tests/normalised_error.py on the CPU: the fp32 oracle's own output stands in for a prediction.

Unperturbed it is inside every bound (by construction: this guards the plumbing, the level keys and the NaN handling on all
seven golden cases).  With an error planted, the pair the model tests held until now (mean-rel <= 1e-4 and max-rel <= 1e-3 over
the whole variable in physical units) still passes -- that is the hole -- and the per-entry check fails and names the
variable, the level and the position.  Amplitudes: 0.01 sigma, between what the old pair allows (0.023 sigma for 2t,
0.085 for msl, 0.124 for z at 850 hPa) and the new bounds (a few 1e-5 sigma).
"""
import pytest
import torch

from aurora_amd import normalisation
from tests import helpers
from tests import normalised_error as ne
from tests.golden_cases import CASES

CASE, LEVELS = "base_pad", CASES["base_pad"]["levels"]
P = helpers.case_model_meta(CASE)[1].config.patch_size
OLD_MEAN, OLD_MAX = 1e-4, 1e-3


def _old_pair_passes(pred, ref):
    """tests/test_gpu_model.py::test_fp32_engine_matches_reference_golden, per variable."""
    return all(helpers.mean_rel_err(pred[k], ref[k]) <= OLD_MEAN and helpers.rel_err(pred[k], ref[k]) <= OLD_MAX for k in ref)


def _stand_in():
    return {k: v.clone() for k, v in ne.oracle_fp32_rollout(CASE)[0].items()}, ne.golden(CASE)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_the_fp32_oracle_is_inside_its_own_bounds_on_every_case_and_step(name):
    case = CASES[name]
    gold = helpers.load_golden(name)
    seen = 0
    for step in range(case["steps"]):
        pred, ref = ne.oracle_fp32_rollout(name)[step], ne.golden(name)[step]
        errors = ne.per_level_errors(pred, ref, case["levels"])
        n_surf = sum(k.startswith("surf.") for k in ref)
        n_atmos = sum(k.startswith("atmos.") for k in ref)
        assert len(errors) == n_surf + n_atmos * len(case["levels"])            # one entry per variable and level
        assert all(k in normalisation.scales for k in errors)
        assert ne.check_fp32(f"{name} step {step} oracle", pred, name, step) <= 1.0
        for e in errors.values():
            assert 0 < e.floor < 1e-4 and 0 <= e.mean <= e.max < 1e-2 and e.flipped <= ne.FLIPPED_CAP
        seen += len(ref)
    assert seen == len(gold)
    if name == "wave":     # NaN over land: the entries are taken over the finite points only, and the masks agree
        assert torch.isnan(ne.golden(name)[0]["surf.swh"]).any()


def test_entries_positions_and_nan_handling_on_a_hand_made_field():
    ref = {"surf.msl": torch.full((2, 1, 3, 5), 1e5), "atmos.t": torch.full((2, 1, 2, 3, 5), 250.0)}
    pred = {k: v.clone() for k, v in ref.items()}
    pred["surf.msl"][1, 0, 2, 4] += 3 * normalisation.scales["msl"]
    pred["atmos.t"][0, 0, 1, 1, 3] -= 2 * normalisation.scales["t_850"]
    pred["atmos.t"][1, 0, 1, 0, 0] += 1 * normalisation.scales["t_850"]
    e = ne.per_level_errors(pred, ref, (500, 850))
    assert set(e) == {"msl", "t_500", "t_850"}
    assert e["msl"].where == (1, 0, 2, 4) and e["msl"].max == pytest.approx(3, rel=1e-4) and e["msl"].mean == pytest.approx(3 / 30, rel=1e-4)
    assert e["t_850"].where == (0, 0, 1, 3) and e["t_850"].max == pytest.approx(2, rel=1e-4) and e["t_850"].mean == pytest.approx(3 / 30, rel=1e-4)
    assert e["t_500"].max == 0 and e["t_500"].flipped == 0
    assert e["msl"].floor == pytest.approx(2.0 ** -7 / normalisation.scales["msl"], rel=1e-12)     # fp32 ulp of 1e5: 2^(16 - 23)
    assert e["t_850"].floor == pytest.approx(2.0 ** -16 / normalisation.scales["t_850"], rel=1e-12)  # of 250: 2^(7 - 23)
    # NaN where both have it is no error; a NaN on one side only counts as flipped and stays out of the values
    ref["surf.msl"][0, 0, 0, 0] = float("nan")
    pred["surf.msl"][0, 0, 0, 0] = float("nan")
    pred["surf.msl"][0, 0, 0, 1] = float("nan")
    e = ne.per_level_errors(pred, ref, (500, 850))
    assert e["msl"].flipped == pytest.approx(1 / 30) and e["msl"].where == (1, 0, 2, 4) and e["msl"].mean == pytest.approx(3 / 28, rel=1e-4)
    bad = ne.failures(e, ne.bounds(ne.per_level_errors(ref, ref, (500, 850))))
    assert [line.split(":")[0] for line in bad] == ["msl", "msl", "t_850"] and "NaN masks differ" in bad[0]
    assert "(1, 0, 2, 4)" in bad[1] and "(0, 0, 1, 3)" in bad[2]


def _assert_hidden_from_the_old_pair_and_named_by_the_new(pred, ref, keys, position):
    assert _old_pair_passes(pred, ref)                                           # the hole
    errors = ne.per_level_errors(pred, ref, LEVELS)
    bad = ne.failures(errors, ne.fp32_bounds(CASE, 0))
    assert sorted(line.split(":")[0] for line in bad) == sorted(keys), bad       # these entries and no other
    for k in keys:
        assert position(errors[k].where), (k, errors[k].where)
    with pytest.raises(AssertionError, match=keys[0]):
        ne.check_fp32("planted", pred, CASE, 0)


def test_a_humidity_head_that_emits_only_its_location_is_caught_at_100_hpa():
    pred, ref = _stand_in()
    pred["atmos.q"][:, :, 0] = normalisation.locations["q_100"]
    _assert_hidden_from_the_old_pair_and_named_by_the_new(pred, ref, ["q_100"], lambda w: True)
    assert ne.per_level_errors(pred, ref, LEVELS)["q_100"].max > 1.0             # sigmas, where the bound is ~1e-5


def test_one_patch_of_z_at_850_hpa():
    pred, ref = _stand_in()
    rows, cols = slice(5 * P, 6 * P), slice(17 * P, 18 * P)
    pred["atmos.z"][0, 0, 3, rows, cols] += 0.01 * normalisation.scales["z_850"]
    _assert_hidden_from_the_old_pair_and_named_by_the_new(
        pred, ref, ["z_850"], lambda w: w[:2] == (0, 0) and rows.start <= w[2] < rows.stop and cols.start <= w[3] < cols.stop)


def test_the_last_latitude_row_of_msl():
    pred, ref = _stand_in()
    pred["surf.msl"][..., -1, :] += 0.01 * normalisation.scales["msl"]
    _assert_hidden_from_the_old_pair_and_named_by_the_new(pred, ref, ["msl"], lambda w: w[2] == ref["surf.msl"].shape[-2] - 1)


def test_the_first_longitude_column_of_2t():
    pred, ref = _stand_in()
    pred["surf.2t"][..., 0] += 0.01 * normalisation.scales["2t"]
    _assert_hidden_from_the_old_pair_and_named_by_the_new(pred, ref, ["2t"], lambda w: w[3] == 0)


def test_a_term_of_the_temperature_head_in_reversed_level_order():
    """A whole variable with its levels reversed is the wrong example: the fields are O(1) sigma and differ between levels, so
    the old pair sees it (t: mean-rel 4.5e-2, max-rel 1.2e-1; every other variable more).  What it does not see is a small
    term of a head with the wrong level stride: here 1e-3 of the head's normalised output lands on the mirrored level, under
    the right location / scale tables -- up to about 0.01 sigma, on every level of t and on nothing else."""
    pred, ref = _stand_in()
    n = normalisation.normalise_atmos_var(pred["atmos.t"].double(), "t", LEVELS)
    assert not _old_pair_passes({"atmos.t": normalisation.unnormalise_atmos_var(n.flip(2), "t", LEVELS).float()}, {"atmos.t": ref["atmos.t"]})
    n = n + 1e-3 * (n.flip(2) - n)
    pred["atmos.t"] = normalisation.unnormalise_atmos_var(n, "t", LEVELS).float()
    keys = [f"t_{lv}" for lv in LEVELS]
    _assert_hidden_from_the_old_pair_and_named_by_the_new(pred, ref, keys, lambda w: True)
    e = ne.per_level_errors(pred, ref, LEVELS)
    assert all(1e-3 < e[k].max < 2e-2 for k in keys)
    assert e["t_100"].max == pytest.approx(e["t_850"].max, rel=1e-2) and e["t_250"].max == pytest.approx(e["t_500"].max, rel=1e-2)


def test_autocast_bounds_are_never_tighter_than_the_fp32_bounds():
    b16 = ne.bounds(ne.oracle_autocast_errors(CASE, 0), margin=3.0, floor=ne.fp32_bounds(CASE, 0))
    b32 = ne.fp32_bounds(CASE, 0)
    assert all(b16[k][0] >= b32[k][0] and b16[k][1] >= b32[k][1] for k in b32)
    worst = max(b16[k][0] for k in b16)
    assert worst < 0.5, worst          # sigmas: bf16 through the backbone, still far below an O(1) sigma field


@pytest.mark.parametrize("name", list(CASES))
def test_where_the_handles_own_tables_are_other_inputs_than_the_goldens(name):
    """A handle given lat / lon alone derives its position / scale tables through libm where the reference goes through torch's
    fp32 kernels (host-only code, compared here without a GPU).  Measured on an EPYC host: on the grids of lora_all and
    air_pollution some patch root areas land on another fp32 value and the shortest scale wavelengths turn that into O(1)
    differences of sin / cos (max 1.99 / 1.89, in 16 of 32 / 49 of 128 patches); on the other five golden grids the tables are
    equal to 2e-9.  Which grids differ is a property of the host's libm and torch build, so it is printed, and what is
    asserted follows the measured difference.  Where they differ, a forecast on them is held against the
    oracle on the same tables (`check_own_tables`), whose fp32 run is inside its own bound there like anywhere else; where they
    do not, that reference is the golden's to fp32 rounding."""
    import torch

    from oracle import aurora_oracle as oracle

    case, model = helpers.case_model_meta(name)
    cfg = model.config
    lat, lon = helpers.case_inputs(case, cfg)[3:5]
    lat = lat[:len(lat) - len(lat) % cfg.patch_size]
    pos, scale = ne.handle_tables(cfg.embed_dim, lat, lon, cfg.patch_size)
    pos_t, scale_t = oracle.pos_scale_encodings(cfg.embed_dim, lat.float(), lon.float(), cfg.patch_size)
    assert pos.shape == pos_t.shape and scale.shape == scale_t.shape
    assert (pos - pos_t).abs().max() < 1e-6                      # positions: equal everywhere
    differ = (scale - scale_t).abs().max().item()
    patches = int(((scale - scale_t).abs().amax(dim=1) > 1e-3).sum())
    print(name, "scale tables: max difference", differ, "patches that differ", patches, "of", scale.shape[0])
    assert differ <= 2.0 and (differ < 1e-6) == (patches == 0)
    long_waves = slice(3 * cfg.embed_dim // 8, cfg.embed_dim // 2)   # wavelengths from ~1e5 km^2 up: far above one ulp of a root
    assert (scale - scale_t)[:, long_waves].abs().max() < 1e-5
    for step in range(case["steps"]):
        like, plain = ne.own_tables_errors(name, step), ne.oracle_fp32_errors(name, step)
        assert set(like) == set(plain)
        own64 = ne.oracle_rollout(name, torch.float64, False, True)[step]
        assert ne.check(f"{name} step {step}, fp32 oracle on the handle's tables", ne.oracle_rollout(name, torch.float32, False, True)[step],
                        own64, case["levels"], like) <= 1.0
        if differ < 1e-6:                                           # the same inputs: the fp64 oracle on them is the golden
            ne.check_fp32(f"{name} step {step}, fp64 oracle on the handle's tables", own64, name, step)
