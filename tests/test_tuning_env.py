"""The AURORA_* switches as `aurora_amd/engine/lib.py:tuning_from_env` hands them to the library: 0 in a field is
"the library's default", so a value the function does not understand must be an error that names the variable -- never the
default, or a test that flips a switch would compare a path with itself.
"""
import pytest

from aurora_amd.engine import lib

SWITCHES = {"AURORA_BAND_SPLIT_ATTENTION": "band_split_attention", "AURORA_QKV_PLANES": "qkv_planes", "AURORA_SPLIT_K": "split_k",
            "AURORA_PERCEIVER_REASSOC": "perceiver_reassoc", "AURORA_SCORE_WEIGHTS": "score_weights"}
FIELDS = ("fuse_ln", *SWITCHES.values())


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in ("AURORA_FUSE_LN", *SWITCHES):
        monkeypatch.delenv(var, raising=False)


def fields(t):
    return {f: getattr(t, f) for f in FIELDS}


def test_unset_variables_leave_every_field_at_the_library_default():
    assert fields(lib.tuning_from_env()) == dict.fromkeys(FIELDS, 0)


@pytest.mark.parametrize("var", sorted(SWITCHES))
def test_switch_accepts_0_and_1_and_touches_only_its_own_field(monkeypatch, var):
    for raw, code in (("0", 1), ("1", 2), (" 1 ", 2)):          # 1: off, 2: on (0 is "default")
        monkeypatch.setenv(var, raw)
        assert fields(lib.tuning_from_env()) == {**dict.fromkeys(FIELDS, 0), SWITCHES[var]: code}, raw


def test_fuse_ln_accepts_0_1_2(monkeypatch):
    for raw, code in (("0", 1), ("1", 2), ("2", 3)):            # never / fill rule / always
        monkeypatch.setenv("AURORA_FUSE_LN", raw)
        assert fields(lib.tuning_from_env()) == {**dict.fromkeys(FIELDS, 0), "fuse_ln": code}


@pytest.mark.parametrize("var,raw", [(v, r) for v in sorted(SWITCHES) for r in ("2", "-1", "", "on", "true", "1.0", "0x1")]
                         + [("AURORA_FUSE_LN", r) for r in ("3", "-1", "", "always", "2.0")])
def test_value_outside_the_range_is_an_error_that_names_the_variable(monkeypatch, var, raw):
    monkeypatch.setenv(var, raw)
    with pytest.raises(ValueError, match=var):
        lib.tuning_from_env()
