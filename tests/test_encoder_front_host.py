"""The encoder front composed, host side (no device): the pack-time composition against fp64 `torch` products of the same
tensors, the compose-or-not rule, and the guard bound recomputed from the composed value rows against the one the two
stages gave (include/aurora_hip.h: aurora_hip_compose_weight / _compose_bias / _compose_front_rule / _composed_value_bound).
"""
import ctypes

import pytest
import torch

import aurora_amd
from aurora_amd.engine import lib
from tests import helpers

F16_SAFE = 16384.0


def _ptr(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def _compose(w_ctx, w_e, bias):
    """(W_c (groups, N, K), bias rows (C, N)) as the library composes them."""
    (N, D), (G, _, K), C = w_ctx.shape, w_e.shape, bias.shape[0]
    w, b = torch.empty(G, N, K), torch.empty(C, N)
    L = lib.load()
    assert L.aurora_hip_compose_weight(_ptr(w_ctx), N, D, _ptr(w_e), K, G, _ptr(w)) == 0
    assert L.aurora_hip_compose_bias(_ptr(w_ctx), N, D, _ptr(bias), C, _ptr(b)) == 0
    return w, b


@pytest.mark.parametrize("groups", [1, 3])
def test_composed_weight_and_bias_equal_fp64_products_to_fp32_rounding(groups):
    """Odd sizes, several groups: every element is the fp64 product rounded once -- at most half an ulp from it, where an
    fp32-accumulated product of D = 70 terms would be several."""
    g = torch.Generator().manual_seed(groups)
    N, D, K, C = 37, 70, 96, 5
    w_ctx, w_e, bias = torch.randn(N, D, generator=g), torch.randn(groups, D, K, generator=g), torch.randn(C, D, generator=g)
    w, b = _compose(w_ctx, w_e, bias)
    w64 = torch.einsum("nd,gdk->gnk", w_ctx.double(), w_e.double())
    b64 = bias.double() @ w_ctx.double().T
    assert ((w.double() - w64).abs() <= 2.0 ** -24 * w64.abs() + 1e-45).all()
    assert ((b.double() - b64).abs() <= 2.0 ** -24 * b64.abs() + 1e-45).all()
    L = lib.load()
    assert L.aurora_hip_compose_weight(None, N, D, _ptr(w_e), K, groups, _ptr(w)) == -1
    assert L.aurora_hip_compose_bias(_ptr(w_ctx), 0, D, _ptr(bias), C, _ptr(b)) == -1


def _rule(Kpad, D, N):
    arr = (ctypes.c_int32 * len(N))(*N)
    return bool(lib.load().aurora_hip_compose_front_rule(Kpad, D, arr, len(N)))


def test_rule_composes_patch_size_4_and_declines_patch_size_10():
    """2 sum Kpad N <= Kpad D + sum D N: at most half the multiply-adds of the stages replaced."""
    assert _rule(160, 512, [768])             # 0.25 degree, patch size 4, [W_v | scores]: 0.26 of the work
    assert _rule(160, 256, [512])             # the small model: 0.48
    assert _rule(256, 512, [768])             # air pollution (patch size 3, 13 variables): 0.38
    assert not _rule(1000, 512, [768])        # patch size 10: 0.85
    assert not _rule(1000, 256, [512])
    assert not _rule(160, 64, [128])          # the golden cases' width: the embedding is the cheap stage there
    # the threshold itself, and a deeper resampler whose layers all read the context: the embedding is paid once
    assert _rule(384, 512, [768]) and not _rule(385, 512, [768])
    assert _rule(160, 512, [768, 1024]) and not _rule(1000, 512, [768, 1024])
    assert not _rule(160, 512, []) and not _rule(0, 512, [768]) and not _rule(160, 512, [0])


def test_recomputed_guard_bound_is_never_looser_on_the_fixtures_weights():
    """|v| <= a w + c for the attention's value rows (w = max |normalised input|).  The two stages gave a = v_l1 l1_e,
    c = v_l1 max|b|; the composed value rows give their own largest L1 row norm and bias maximum.  The induced norm is
    submultiplicative, so the new bound is at most the old one for every w -- on the deterministic weights of the fixtures
    strictly smaller --, and the limit it puts on w admits everything the old limit admitted."""
    with torch.device("meta"):
        meta = aurora_amd.Aurora(embed_dim=256, num_heads=8, encoder_depths=(2, 2, 2), encoder_num_heads=(4, 8, 16),
                                 decoder_depths=(2, 2, 2), decoder_num_heads=(16, 8, 4))
    sd = helpers.case_state_dict(meta, torch.float32)
    D, T, P = 256, 2, 4
    w_e = torch.cat([sd[f"encoder.atmos_token_embeds.weights.{v}"][:, 0, :T].reshape(D, -1) for v in meta.config.atmos_vars], 1)
    w_kv = sd["encoder.level_agg.layers.0.0.to_kv.weight"]
    w_v = w_kv[w_kv.shape[0] // 2:].contiguous()
    bias = (sd["encoder.atmos_token_embeds.bias"] + torch.randn(4, D, generator=torch.Generator().manual_seed(0))).contiguous()
    assert w_e.shape == (D, 5 * T * P * P)
    w_c, b_c = _compose(w_v, w_e[None].contiguous(), bias)
    l1 = lambda m: float(m.abs().sum(-1).max())  # noqa: E731
    out = (ctypes.c_float * 6)()
    assert lib.load().aurora_hip_composed_value_bound(l1(w_v), l1(w_e), float(bias.abs().max()), l1(w_c[0]),
                                                      float(b_c.abs().max()), out) == 0
    a_old, c_old, lim_old, a_new, c_new, lim_new = out
    print(f"|v| <= {a_old:.4g} w + {c_old:.4g} (two stages, w < {lim_old:.4g}); <= {a_new:.4g} w + {c_new:.4g} (composed, w < {lim_new:.4g})")
    assert 0 < a_new < a_old and 0 <= c_new < c_old
    assert lim_old <= lim_new <= F16_SAFE / a_new
    # composed norms ABOVE the stages' (rounding, or a caller's mistake) never loosen it: the stages' bound is kept
    assert lib.load().aurora_hip_composed_value_bound(2.0, 3.0, 1.0, 7.0, 5.0, out) == 0
    assert (out[3], out[4]) == (6.0, 2.0) and out[5] == float(torch.tensor(F16_SAFE - 2.0) / 6.0)   # (float32, as the library divides)
    assert lib.load().aurora_hip_composed_value_bound(0.0, 3.0, 1.0, 7.0, 5.0, out) == -1
