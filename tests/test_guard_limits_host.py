"""The limits a step compares its guard words against, host side (no device): every quantity they are made of recomputed in fp64
from the state dict, and the engine's own numbers -- recorded results of `aurora_hip_guard_limits`, written by
tests/test_gpu_guard_limits.py into tests/golden/guard_limits.json (the handle derives them while it packs weights on the
device, so they cannot be asked for here) -- held against them.

A limit is SOUND when the two-term kernels it admits never see an operand outside fp16: with w < limit the bound derived for
every guarded launch's activation operand, `limit x (L1 norms) + bias maxima`, followed through every stage of its chain, stays
below 65504.  It is HONEST when it is no larger than the fp64 value of its own formula (csrc/step.hip), up to the rounding of
the engine's float L1 sums (K terms: K 2^-24 relative).
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd.engine import encodings
from tests import helpers
from tests.golden_cases import CASES as GOLDEN

F16_SAFE, F16_MAX = 16384.0, 65504.0
_SMALL = dict(embed_dim=256, num_heads=8, encoder_depths=(2, 2, 2), encoder_num_heads=(4, 8, 16), decoder_depths=(2, 2, 2),
              decoder_num_heads=(16, 8, 4))
CASES = {**{k: GOLDEN[k] for k in ("base_pad", "small_b2", "patch10", "air_pollution")},
         "chain256": dict(cls="Aurora", kwargs=dict(**_SMALL), H=16, W=32, B=1, T=2, levels=(100, 250, 500, 850))}
RECORDED = json.loads((Path(__file__).parent / "golden" / "guard_limits.json").read_text())


def _l1(w):
    return float(w.double().abs().sum(-1).max())


def _no_larger(engine, exact, terms):
    """engine <= exact, up to the rounding of a float sum of `terms` magnitudes the engine's limit divides by."""
    return engine <= exact * (1 + terms * 2.0 ** -24)


def _value_rows(sd, prefix):
    """The value halves of to_kv of every layer of a Perceiver."""
    out, i = [], 0
    while f"{prefix}.layers.{i}.0.to_kv.weight" in sd:
        w = sd[f"{prefix}.layers.{i}.0.to_kv.weight"]
        out.append(w[w.shape[0] // 2:])
        i += 1
    assert out
    return out


def _state(name):
    case = CASES[name]
    with torch.device("meta"):
        meta = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    return case, meta, helpers.case_state_dict(meta, torch.float32)


@pytest.mark.parametrize("name", ["base_pad", "small_b2", "patch10", "air_pollution"])
def test_context_limits_of_the_golden_cases(name):
    """64 wide: the encoder front is no guarded chain, so the encoder (word 0) and decoder (word 3) Perceivers each measure
    their own context.  The context linear reads it directly (limit F16_SAFE); the attention output is a convex combination of
    value rows, |att| <= max |v| <= v_l1 max |ctx|, so to_out's limit is F16_SAFE / v_l1."""
    case, meta, sd = _state(name)
    rec = RECORDED[f"{name}/composed"]
    assert rec["limits"][1] is None and rec["limits"][2] is None and rec["launches"][1] == rec["launches"][2] == 0
    decoders = ["decoder.level_decoder"] + (["decoder.level_decoder_alternate"] if "decoder.level_decoder_alternate.layers.0.0.to_kv.weight" in sd else [])
    for word, prefixes in ((0, ["encoder.level_agg"]), (3, decoders)):
        limit = rec["limits"][word]
        assert limit is not None and rec["launches"][word] > 0 and 0 < limit <= F16_SAFE
        exact = F16_SAFE
        for prefix in prefixes:
            for w_v in _value_rows(sd, prefix):
                v_l1 = _l1(w_v)
                exact = min(exact, F16_SAFE / v_l1)
                assert limit * v_l1 < F16_MAX, (prefix, limit, v_l1)          # to_out's operand
        print(f"{name} word {word}: engine {limit!r}, fp64 {exact!r}")
        assert _no_larger(limit, exact, max(w.shape[1] for p in prefixes for w in _value_rows(sd, p)))


def _front(sd, meta, case):
    """fp64 quantities of the D = 256 case's encoder front."""
    T, D = case["T"], meta.config.embed_dim
    w_e = torch.cat([sd[f"encoder.atmos_token_embeds.weights.{v}"][:, 0, :T].reshape(D, -1) for v in meta.config.atmos_vars], 1).double()
    lv = torch.from_numpy(np.asarray(encodings.levels(case["levels"], D), dtype=np.float64))
    enc_bias = (lv @ sd["encoder.atmos_levels_embed.weight"].double().T + sd["encoder.atmos_levels_embed.bias"].double()
                + sd["encoder.atmos_token_embeds.bias"].double())                                  # (C, D)
    w_s = torch.cat([w[:, 0, :T].reshape(D, -1) for k, w in sd.items() if k.startswith("encoder.surf_token_embeds.weights.")], 1)
    return dict(w_e=w_e, l1_e=_l1(w_e), cb=float(enc_bias.abs().max()), enc_bias=enc_bias, l1_s=_l1(w_s),
                surf_c=float(sd["encoder.surf_token_embeds.bias"].abs().max()) + float(sd["encoder.surf_level_encoding"].abs().max()),
                surf_l1_0=_l1(sd["encoder.surf_mlp.net.0.weight"]), surf_b0=float(sd["encoder.surf_mlp.net.0.bias"].abs().max()),
                K_s=w_s.shape[1])


def test_surface_chain_limit_follows_both_stages():
    """Word 2 = max |normalised surface input| w.  Embedding: the input itself.  First MLP linear: |xs0| <= l1_e w + c, with
    c = max |patch bias| + max |level encoding|.  Second: |GELU(h)| <= |h| <= l1_0 (l1_e w + c) + max |b0|."""
    case, meta, sd = _state("chain256")
    f = _front(sd, meta, case)
    for key in ("chain256/composed", "chain256/staged"):
        limit = RECORDED[key]["limits"][2]
        assert RECORDED[key]["launches"][2] == 6 and 0 < limit <= F16_SAFE
        xs0 = limit * f["l1_s"] + f["surf_c"]
        hid = xs0 * f["surf_l1_0"] + f["surf_b0"]
        lim_0 = (F16_SAFE - f["surf_c"]) / f["l1_s"]
        lim_2 = ((F16_SAFE - f["surf_b0"]) / f["surf_l1_0"] - f["surf_c"]) / f["l1_s"]
        print(f"{key} word 2: engine {limit!r}; fp64 lim_0 {lim_0!r} lim_2 {lim_2!r}; |xs0| <= {xs0:.6g}, |hidden| <= {hid:.6g}")
        assert limit < F16_MAX and xs0 < F16_MAX and hid < F16_MAX
        assert _no_larger(limit, min(F16_SAFE, lim_0, lim_2), f["K_s"] + 256)


def test_atmospheric_chain_limits_staged_and_composed():
    """Word 1 = max |normalised atmospheric input| w.  Two stages: |x| <= l1_e w + cb for the embeddings (written as fp16 pairs
    and read by to_kv), |att| <= v_l1 (l1_e w + cb).  Composed: the context linear reads the input itself, and
    |att| <= ||W_v W_e||_inf w + max |W_v (b_e + level embedding)|, never looser than the product of the stages' norms."""
    case, meta, sd = _state("chain256")
    f = _front(sd, meta, case)
    (w_v,) = _value_rows(sd, "encoder.level_agg")
    v_l1 = _l1(w_v)
    staged, composed = RECORDED["chain256/staged"], RECORDED["chain256/composed"]
    assert not staged["front_composed"] and composed["front_composed"]
    # two stages
    limit = staged["limits"][1]
    x = limit * f["l1_e"] + f["cb"]
    lim_kv, lim_out = min(F16_SAFE, (F16_SAFE - f["cb"]) / f["l1_e"]), (F16_SAFE / v_l1 - f["cb"]) / f["l1_e"]
    print(f"staged word 1: engine {limit!r}; fp64 limit_kv {lim_kv!r} lim_out {lim_out!r}; |x| <= {x:.6g}, |att| <= {v_l1 * x:.6g}")
    assert 0 < limit <= F16_SAFE and x < F16_MAX and v_l1 * x < F16_MAX
    assert _no_larger(limit, min(lim_kv, lim_out), f["w_e"].shape[1] + w_v.shape[1])
    # composed
    limit_c = composed["limits"][1]
    w_c = w_v.double() @ f["w_e"]
    a, c = _l1(w_c), float((f["enc_bias"] @ w_v.double().T).abs().max())
    assert a <= v_l1 * f["l1_e"] and c <= v_l1 * f["cb"]                      # the induced norm is submultiplicative
    print(f"composed word 1: engine {limit_c!r}; fp64 (F16_SAFE - {c:.6g}) / {a:.6g} = {(F16_SAFE - c) / a!r}; |att| <= {limit_c * a + c:.6g}")
    assert 0 < limit_c <= F16_SAFE and limit_c * a + c < F16_MAX
    assert _no_larger(limit_c, min(F16_SAFE, (F16_SAFE - c) / a), f["w_e"].shape[1] + w_v.shape[1])
    assert limit <= limit_c                                                    # (admits everything the stages admitted)
    # the encoder ran inside the chain both times: its own word carries nothing; the decoder's is as in the golden cases
    for rec in (staged, composed):
        assert rec["launches"][0] == 0 and rec["limits"][0] is None
        lim3 = rec["limits"][3]
        for w in _value_rows(sd, "decoder.level_decoder"):
            assert lim3 * _l1(w) < F16_MAX
        assert _no_larger(lim3, min(F16_SAFE / _l1(w) for w in _value_rows(sd, "decoder.level_decoder")), 512)
