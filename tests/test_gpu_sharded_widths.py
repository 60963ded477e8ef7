"""The latitude-band step (csrc/step.hip: attention_band, post_halo, attend_behind_halo; block, merge_stage and split_stage on
band-local rows) at the PRODUCTION widths and under every switch that changes its launches.

tests/test_gpu_sharded.py runs bands at embed_dim 64 with 1 / 2 / 4 heads and default tuning only; tests/test_gpu_production.py
runs the production widths, but no band.  Here the two meet: `aurora_amd.Aurora` with embed_dim 512, heads 8 / 16 / 32
(D = 512 / 1024 / 2048), depths cut to (2, 2, 2) / (2, 2, 2) -- one unshifted and one shifted block per stage -- random weights
(`_seeded_model`: the zero-initialised tensors re-randomised), inputs of `bench.synthetic_batch` with four pressure levels.

Grid: 192 x 96 (token grid 4 x 48 x 24), the one tests/test_gpu_sharded.py already splits over 2, 3 and 4 ranks; one fp64 oracle
run of this model (334 M parameters) on it takes 2 s on eight CPU cores, the fp32 run 1 s, so no smaller grid was needed.
Worlds: 2 and 3 -- with 3 ranks the middle one has two neighbours (both halo sides, the `recv_off` adjacency), and 16 / 8 / 4
owned rows per stage are no multiple of the window's 6, so the UNSHIFTED blocks exchange halo rows as well.

Bounds, and where each comes from (no tolerance here is a constant of this module's own):
* fp32 against the oracle in fp64, and stitched against un-sharded: per entry (tests/normalised_error.py) within `ne.MARGIN` of
  what the fp32 oracle deviates from the fp64 oracle by (or of one fp32 ulp of the entry) -- the bound tests/test_gpu_production.py
  holds the un-sharded step to.
* bf16 against the oracle in fp64, and stitched against un-sharded: per entry within 3x of what the oracle's own autocast run
  deviates from the fp64 oracle by, never tighter than the fp32 bound (`ne.check_autocast`'s rule, the bound of
  tests/test_gpu_sharded.py::test_sharded_equals_unsharded), with this module's own oracle runs as the baseline.
* bit equality (`torch.equal`) where two runs do the same arithmetic on the same values: the split attention launch, the
  q | k | v layout, a handle after a refused step, and fp32 bands against the un-sharded step when every handle's range words
  name the same path.

The three oracle runs (fp32, autocast, fp64) are made once per module and shared, read-only.
"""
import ctypes
import dataclasses
import functools
import gc

import pytest
import torch

import aurora_amd
from aurora_amd.batch import BandBatch, derive_metadata
from aurora_amd.engine import geometry, lib
from tests import normalised_error as ne
from tests.test_gpu_production import _inputs, _oracle, _seeded_model
from tests.test_gpu_sharded import host_fields, make, make_engines, run_virtual_ranks, stitch

pytestmark = pytest.mark.gpu

KW = dict(embed_dim=512, num_heads=16, encoder_depths=(2, 2, 2), encoder_num_heads=(8, 16, 32), decoder_depths=(2, 2, 2),
          decoder_num_heads=(32, 16, 8))
H, W = 192, 96
LEVELS = (100, 250, 500, 850)
AUTOCAST_MARGIN = 3.0     # ne.check_autocast's default
SWITCHES = {"fuse": "AURORA_FUSE_LN", "planes": "AURORA_QKV_PLANES", "split": "AURORA_BAND_SPLIT_ATTENTION"}


@dataclasses.dataclass(frozen=True)
class Setup:
    model: object       # on the device; `autocast` is set per run (the handle reads it when it is created)
    batch: object       # on the host
    ref64: dict         # the oracle in fp64 on the same fp32 weights
    bound32: dict       # entry -> (max, mean): ne.MARGIN x what the fp32 oracle deviates from ref64 by (or one fp32 ulp)
    bound16: dict       # entry -> (max, mean): 3 x what the autocast oracle deviates from ref64 by, at least bound32


@functools.lru_cache(maxsize=None)
def _setup() -> Setup:
    model = _seeded_model(aurora_amd.Aurora, autocast=False, **KW)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    batch = _inputs(model.config, H, W, LEVELS)
    ref32 = _oracle(model, sd, batch, autocast=False)
    ref16 = _oracle(model, sd, batch, autocast=True)
    ref64 = _oracle(model, {k: v.double() for k, v in sd.items()}, batch, autocast=False)
    bound32 = ne.bounds(ne.per_level_errors(ref32, ref64, LEVELS))
    bound16 = ne.bounds(ne.per_level_errors(ref16, ref64, LEVELS), margin=AUTOCAST_MARGIN, floor=bound32)
    return Setup(model, batch, ref64, bound32, bound16)


def _within(what, pred, ref, bound):
    """Every entry of pred against ref within its bound (`ne.failures`); prints and returns the worst ratio to the bound."""
    errors = ne.per_level_errors(pred, ref, LEVELS)
    ratio, key = max((max(e.max / bound[k][0], e.mean / bound[k][1]), k) for k, e in errors.items())
    print(f"{what}: worst ratio to the bound {ratio:.3f} ({key})")
    bad = ne.failures(errors, bound)
    assert not bad, f"{what}: " + "; ".join(bad)
    return ratio


def _set(monkeypatch, model, autocast, **switches):
    """The switches are read when a handle is created: every run below creates its handles after this."""
    for k, name in SWITCHES.items():
        monkeypatch.delenv(name, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(SWITCHES[k], v)
    model.autocast = autocast
    model._engine = None


def _whole(model, batch, steps=1):
    """The un-sharded step(s): fields on the host, and the handle's account of its fp32 paths."""
    with torch.inference_mode():
        pred = list(aurora_amd.rollout(model, batch, steps=steps))[-1] if steps > 1 else model.forward(batch)
    torch.cuda.synchronize()
    return host_fields(pred.surf_vars, pred.atmos_vars), _paths(model.engine().native)


def _next_state(engines, model, batch, bands):
    """Every rank's input of the second roll-out step: its band of the newest input state in front of its own prediction."""
    dev = batch.crop(model.patch_size).to("cuda")
    nxt = []
    for r, b in enumerate(bands):
        mine = engines[r].local_band(dev)
        nxt.append(dataclasses.replace(
            b, surf_vars={k: torch.cat([mine.surf_vars[k][:, 1:], v], dim=1) for k, v in b.surf_vars.items()},
            atmos_vars={k: torch.cat([mine.atmos_vars[k][:, 1:], v], dim=1) for k, v in b.atmos_vars.items()}))
        assert isinstance(nxt[-1], BandBatch)
    return nxt


def _bands(model, batch, world, steps=1):
    """`steps` sharded steps on the same engines, the state kept as BandBatches: [the bands of every step], exchanges, engines."""
    engines = make_engines(model, world)
    with torch.inference_mode():
        bands, n_ex = run_virtual_ranks(model, batch, world, engines)
        out = [bands]
        for _ in range(1, steps):
            bands, n = run_virtual_ranks(model, _next_state(engines, model, batch, out[-1]), world, engines)
            n_ex += n
            out.append(bands)
    torch.cuda.synchronize()
    for bs in out:
        assert [b.band for b in bs] == sorted(b.band for b in bs) and bs[0].band[0] == 0
        assert all(isinstance(b, BandBatch) for b in bs)
    return out, n_ex, engines


def _band_fields(bands):
    return [host_fields(b.surf_vars, b.atmos_vars) for b in bands]


def _same_bits(a, b):
    """Per band, per field."""
    assert len(a) == len(b)
    return [(r, k) for r, (x, y) in enumerate(zip(a, b)) for k in x if not torch.equal(x[k], y[k])]


def _paths(native):
    """Which fp32 path every guarded linear of the handle's last step took, as far as the handle tells: per range word that a
    launch carried, (all launches on two fp16 terms?, the word).  A launch runs two terms iff word < its limit, and the handle
    reports the SMALLEST limit per word (aurora_hip_guard_limits), so word < limit names the path of every launch on that word;
    above it the launches' own limits decide, and only the same word means the same paths."""
    words = native.guard_words()
    limits, launches = native.guard_limits()
    return tuple((w < lim, w) if n > 0 else None for w, lim, n in zip(words, limits, launches))


def _paths_differ(handles):
    """The indices of the range words on which the handles may have taken different paths."""
    differ = []
    for i in range(4):
        seen = [h[i] for h in handles]
        assert all((s is None) == (seen[0] is None) for s in seen), (i, seen)   # same launches on every handle
        if seen[0] is not None and not all(s[0] for s in seen) and len({s[1] for s in seen}) > 1:
            differ.append(i)
    return differ


def _free():
    gc.collect()   # a transport and its callbacks refer to each other
    torch.cuda.empty_cache()


# ---- 1. a band equals the whole step, at production widths ------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fuse", ["0", "2"])
@pytest.mark.parametrize("autocast", [False, True])
def test_bands_equal_the_whole_step_and_the_oracle(autocast, fuse, world, monkeypatch):
    """The stitched bands against the un-sharded engine under the same switches and against the oracle in fp64, each within the
    bound of its precision (module docstring).  With AURORA_FUSE_LN=2 the fused linear + AdaLN + residual kernel runs on a
    band-local residual stream and M (0: never); the halo `linear_planes` projection runs with 8 / 16 / 32 heads; the bf16
    linears pick split-K or not for band-local M.

    Measured on an MI355X, worst ratio to the bound (the bound is at 1; 2 and 3 bands give the same figures).  fp32 (the switch
    is a bf16 one): stitched against un-sharded 0.000, both against the oracle 0.471 (v_100).  bf16 fuse_ln 0 / 2: un-sharded
    against the oracle 0.251 / 0.254, stitched against un-sharded 0.188 / 0.174, stitched against the oracle 0.264 / 0.288 (10u)."""
    s = _setup()
    _set(monkeypatch, s.model, autocast, fuse=fuse)
    whole, _ = _whole(s.model, s.batch)
    (bands,), n_ex, _ = _bands(s.model, s.batch, world)
    assert n_ex > 0
    assert all(b.metadata.rollout_step == 1 for b in bands)
    got = host_fields(*stitch(bands))
    assert all(got[k].shape == v.shape for k, v in whole.items())
    bound = s.bound16 if autocast else s.bound32
    what = f"{world} bands autocast={autocast} fuse_ln={fuse}"
    _within(f"{what}, un-sharded against the fp64 oracle", whole, s.ref64, bound)
    _within(f"{what}, stitched against un-sharded", got, whole, bound)
    _within(f"{what}, stitched against the fp64 oracle", got, s.ref64, bound)
    _free()


# ---- 2. fixed fp32 paths give the un-sharded step bit for bit ---------------------------------------------------------------
def test_fp32_bands_are_the_whole_step_bit_for_bit_when_the_paths_agree(monkeypatch):
    """An fp32 band does the arithmetic of the un-sharded step on its own rows -- PROVIDED every large fp32 linear takes the same
    path: those pick two fp16 or three bf16 terms on the device from range words, and a band's words cover its own rows only.
    Where every rank's words name the path of the un-sharded handle (`_paths`) the stitched fields must be `torch.equal`; where
    they do not, the bound of test 1 holds and the word is printed.  The seeded inputs are unit normal in normalised space, far
    inside fp16's range, so every handle takes two terms: the bit-for-bit branch is taken -- asserted, so that it cannot
    silently go unused."""
    s = _setup()
    _set(monkeypatch, s.model, False)
    whole, paths = _whole(s.model, s.batch)
    print(f"un-sharded (two terms on every launch, range word) per word: {paths}")
    assert any(p is not None for p in paths), paths     # the step has guarded linears at all
    bit_for_bit = 0
    for world in (2, 3):
        (bands,), n_ex, engines = _bands(s.model, s.batch, world)
        assert n_ex > 0
        got = host_fields(*stitch(bands))
        rank_paths = [_paths(e.native) for e in engines]
        differ = _paths_differ([paths] + rank_paths)
        print(f"{world} bands per word: {rank_paths}; may differ on {differ}")
        if not differ:
            unequal = [k for k, v in whole.items() if not torch.equal(got[k], v)]
            assert not unequal, (world, unequal, {k: (got[k] - whole[k]).abs().max().item() for k in unequal})
            bit_for_bit += 1
        else:
            print(f"{world} bands: range word(s) {differ} differ between the handles: {paths} / {rank_paths}")
            _within(f"{world} fp32 bands on other paths, stitched against un-sharded", got, whole, s.bound32)
        del engines
        _free()
    assert bit_for_bit > 0


# ---- 3. the split attention launch changes no bit ---------------------------------------------------------------------------
def _plans(cfg, world):
    """(stage, shifted, rank, n_interior, n_windows) of every band plan of the 192 x 96 grid (pure host functions)."""
    L = lib.load()
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    n = len(cfg.encoder_depths)
    res0 = (cfg.latent_levels, H // cfg.patch_size, W // cfg.patch_size)
    out = []
    for stage, res in enumerate(geometry.stage_resolutions(res0, n)[0]):
        rows = []
        for r in range(world):
            h0, h1 = ctypes.c_int32(), ctypes.c_int32()
            lib._check(L.aurora_hip_band_partition(n, i32(res0), i32(cfg.window_size), world, r, stage, ctypes.byref(h0), ctypes.byref(h1)))
            rows += [h0.value, h1.value]
        for shifted in (0, 1):
            for r in range(world):
                info = lib.HipPlanInfo()
                lib._check(L.aurora_hip_band_plan(i32(res), i32(cfg.window_size), shifted, world, r, i32(rows), ctypes.byref(info),
                                                  None, None, None, None))
                out.append((stage, shifted, r, info.n_interior, info.n_windows))
    return out


def _split_flavours(cfg, world):
    """The block flavours (0 unshifted, 1 shifted) in which some rank at some stage runs TWO launches under the split."""
    return {shifted for _, shifted, _, n_int, n_win in _plans(cfg, world) if 0 < n_int < n_win}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("widths", ["production", "base_pad"])
def test_split_attention_launch_changes_no_bit(widths, autocast, world, monkeypatch):
    """AURORA_BAND_SPLIT_ATTENTION=1 runs a band's interior windows in front of the halo `wait` and the others behind the halo
    projection, from offset token / group tables: the same arithmetic on the same values in two launches.  Every field of every
    band must be `torch.equal` to the one-launch run -- at the production widths and on the tiny `base_pad` (many windows, thin
    bands), in two consecutive steps on the same engines: in the second the halo region of `qkv` holds the previous block's
    rows, so a window wrongly ordered into the interior group would read plausible stale values there.

    Precondition, from the band plans: some rank at some stage has 0 < n_interior < n_windows in a shifted block (each world)
    and in an unshifted block (three ranks: their rows are no multiple of the window) -- else one launch would be compared with
    itself."""
    if widths == "production":
        s = _setup()
        model, batch = s.model, s.batch
    else:
        model, batch = make("base_pad", autocast, H, W)
    assert 1 in _split_flavours(model.config, world)
    assert {0, 1} <= _split_flavours(model.config, 2) | _split_flavours(model.config, 3)
    assert world != 3 or _split_flavours(model.config, 3) == {0, 1}
    runs = {}
    for split in ("0", "1"):
        _set(monkeypatch, model, autocast, split=split)
        steps, n_ex, _ = _bands(model, batch, world, steps=2)
        assert n_ex > 0
        runs[split] = [_band_fields(bands) for bands in steps]
        _free()
    for step in (0, 1):
        assert not _same_bits(runs["0"][step], runs["1"][step]), step
    # the second step is another computation than the first (not a replay of its buffers)
    assert all(not torch.equal(a[k], b[k]) for a, b in zip(runs["1"][0], runs["1"][1]) for k in a)


# ---- 4. the qkv layout changes no bit in a band -----------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("fuse", ["0", "2"])
def test_qkv_layout_changes_no_bit_in_a_band(fuse, world, monkeypatch):
    """tests/test_gpu_production.py::test_attention_layouts_give_the_same_prediction_bit_for_bit on bands: with
    AURORA_QKV_PLANES=0 a bf16 band projects its halo rows into rows of 3 dim (the `else if (n_recv > 0)` branch of
    attend_behind_halo with 2-byte elements), with 1 into every head's plane at (Ls + first) * 192 + 64, planes Lq * 192 apart --
    with 8 / 16 / 32 heads a wrong offset, stride or head count cannot hide.  Same values, same arithmetic: `torch.equal`."""
    s = _setup()
    runs = {}
    for planes in ("1", "0"):
        _set(monkeypatch, s.model, True, fuse=fuse, planes=planes)
        (bands,), n_ex, _ = _bands(s.model, s.batch, world)
        assert n_ex > 0
        runs[planes] = _band_fields(bands)
        _free()
    assert not _same_bits(runs["1"], runs["0"])


# ---- 5. a batch of two is refused -------------------------------------------------------------------------------------------
def test_a_band_refuses_a_batch_of_two_and_runs_on():
    """Under autocast with head planes a band holds one batch element (plane_stride = Lq * 192 has no batch axis), and
    attention_band says so ("a latitude band runs one batch element") -- but B = 2 is refused EARLIER, for every sharded step:
    aurora_hip_step (csrc/model.hip) checks "latitude-band sharding runs one forecast (batch size 1) across the ranks" in front
    of the sizing pass, so the REQUIRE in attention_band is a second line that no caller of the C ABI can reach.  The message
    asserted here is therefore the earlier one.  Nothing is enqueued before it: the prediction tensors handed in keep their
    fill, and no halo message is posted.  include/aurora_hip.h does not call a handle unusable after an error, so the SAME
    engines then run a B = 1 step, bit for bit what fresh engines give (the same launches).  `small_b2` (tiny widths, batch of
    two) on the 192 x 96 grid: its own 17 x 32 grid has one token row at the coarsest stage, which no two ranks can share."""
    model, batch = make("small_b2", True, H, W)
    world = 2
    assert next(iter(batch.surf_vars.values())).shape[0] == 2
    engines = make_engines(model, world)
    dev = batch.crop(model.patch_size).to("cuda")
    fill = 12345.0
    outs = []
    for e in engines:
        band = e.local_band(dev)
        outs.append(({k: torch.full_like(v[:, :1], fill) for k, v in band.surf_vars.items()},
                     {k: torch.full_like(v[:, :1], fill) for k, v in band.atmos_vars.items()}))
    hub = engines[0].native.transport.hub
    with pytest.raises(ValueError, match=r"latitude-band sharding runs one forecast \(batch size 1\) across the ranks"):
        run_virtual_ranks(model, batch, world, engines, outs=outs)
    torch.cuda.synchronize()
    assert hub.exchanges == 0 and all(b.empty() for b in hub.boxes.values())
    assert all((t == fill).all() for o in outs for d in o for t in d.values())
    one = dataclasses.replace(batch, surf_vars={k: v[:1] for k, v in batch.surf_vars.items()},
                              atmos_vars={k: v[:1] for k, v in batch.atmos_vars.items()},
                              metadata=derive_metadata(batch.metadata, time=batch.metadata.time[:1]))
    with torch.inference_mode():
        after, n_ex = run_virtual_ranks(model, one, world, engines)
        fresh, _ = run_virtual_ranks(model, one, world)
    torch.cuda.synchronize()
    assert n_ex > 0
    assert not _same_bits(_band_fields(after), _band_fields(fresh))
    assert all(torch.isfinite(v).all() for f in _band_fields(after) for v in f.values())


# ---- 6. a sharded bf16 roll-out of two steps --------------------------------------------------------------------------------
def test_sharded_bf16_rollout_stays_distributed(monkeypatch):
    """tests/test_gpu_sharded.py::test_sharded_rollout_stays_distributed under autocast at these widths with the fused
    linear + AdaLN kernel on: the state kept as BandBatches, step 2 stitched against the un-sharded two-step roll-out within the
    bf16 bound of test 1."""
    s = _setup()
    _set(monkeypatch, s.model, True, fuse="2")
    whole, _ = _whole(s.model, s.batch, steps=2)
    steps, n_ex, _ = _bands(s.model, s.batch, 2, steps=2)
    assert n_ex > 0
    assert all(b.metadata.rollout_step == 2 for b in steps[1])
    _within("2 bands autocast fuse_ln=2, second step, stitched against un-sharded", host_fields(*stitch(steps[1])), whole, s.bound16)
    _free()
