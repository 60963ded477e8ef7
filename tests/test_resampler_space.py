"""The workspace layout of a resampler layer (aurora_amd/csrc/resampler_space.h) replayed on the host: tests/resampler_space_check.cpp
is compiled with g++ as its own program, walks the launches of `resampler` (csrc/step.hip) in order and checks, for every level
count 1..13 of the decoder's de-aggregation (Lq levels, 3 keys) and the encoder's aggregation (3 queries, Lk levels), at the
Perceiver widths of both published sizes, with score weights and re-association on and off, for the first and a later layer,
1..7,200 columns and batch 1 and 2, that no launch writes over what it reads or over what is still live and that every range
stays inside its region.  The widths come from the constructors, not from this file.
"""
import subprocess
from pathlib import Path

import torch

import aurora_amd

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "resampler_space_check.cpp"
CSRC = ROOT / "aurora_amd" / "csrc"


def perceiver_widths(cls):
    """(dim, inner, heads, hidden, side) of the encoder's and the decoder's Perceiver of `cls()`, from its parameters."""
    with torch.device("meta"):
        model = cls()
    sd, heads = model.state_dict(), model.config.num_heads
    out = []
    for side, prefix in (("enc", "encoder.level_agg"), ("dec", "decoder.level_decoder")):
        inner, dim = sd[f"{prefix}.layers.0.0.to_q.weight"].shape
        assert sd[f"{prefix}.layers.0.0.to_out.weight"].shape == (dim, inner)
        hidden = sd[f"{prefix}.layers.0.1.net.0.weight"].shape[0]
        out.append((dim, inner, heads, hidden, side))
    return out


def build_check(out_dir: Path, include: Path = CSRC) -> Path:
    exe = out_dir / "resampler_space_check"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{include}", str(SRC), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_published_perceiver_widths():
    """What the sweep below runs on -- and `inner == dim` in all four, which is what lets the attention output live in the
    result region (`att_in_y`) and the re-associated path exist."""
    assert perceiver_widths(aurora_amd.AuroraPretrained) == [(512, 512, 16, 2048, "enc"), (1024, 1024, 16, 2048, "dec")]
    assert perceiver_widths(aurora_amd.AuroraSmallPretrained) == [(256, 256, 8, 1024, "enc"), (512, 512, 8, 1024, "dec")]


def run_check(exe, widths):
    res = subprocess.run([str(exe), *(",".join(map(str, w)) for w in widths)], capture_output=True, text=True, timeout=120)
    print(res.stdout[-4000:])
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-4000:], res.stderr[-2000:])
    summary = res.stdout.strip().splitlines()[-1]
    assert summary.endswith(": 0 violations"), summary
    keys = ("tuples", "reassoc", "scores", "chunked", "att_in_s")
    return dict(zip(keys, (int(tok) for tok in summary.replace("(", " ").split() if tok.isdigit())))


def test_no_launch_of_the_resampler_writes_over_live_workspace(tmp_path):
    exe = build_check(tmp_path)
    widths = perceiver_widths(aurora_amd.AuroraPretrained) + perceiver_widths(aurora_amd.AuroraSmallPretrained)
    n = run_check(exe, widths)
    # 13 level counts x {scores, re-association, pre-split weights} on / off x 2 layers x 5 column counts x 2 batch sizes,
    # the encoder's also with and without the key LayerNorm
    assert n["tuples"] == 2 * 13 * 8 * 2 * 5 * 2 * (2 + 1), n
    # the sweep met every path of the layout that the published widths reach
    assert n["reassoc"] > 0 and n["scores"] > 0 and n["chunked"] > 0 and n["att_in_s"] == 0, n
    # a Perceiver with inner > dim (none is published): the attention output moves behind k | v | q in the scratch region
    n = run_check(exe, [(256, 512, 8, 1024, "enc"), (512, 1024, 16, 1024, "dec")])
    assert n["att_in_s"] == n["tuples"] and n["reassoc"] == 0, n
    for args in ([], ["512,512,16"], ["512,500,16,2048,dec"], ["512,512,16,2048,mid"]):   # malformed widths
        res = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        assert res.returncode == 2 and "usage:" in res.stderr, args
