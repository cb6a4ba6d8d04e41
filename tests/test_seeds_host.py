"""Per-sample noise seeds, host side (no GPU): the stream-id layout, `vary_seeds`, the rank slice of the global seed list,
the errors of `MultiScaleGaussianDiffusion.sample_seeds`, the command line's seed flags, and the argument validation of
sinddm_normal_fill_samples / sinddm_sample_chain_seeds that happens before any device work."""
import ctypes as C
import os
import sys

import pytest
import torch

from sinddm_amd import _lib
from sinddm_amd import dist as sdist
from sinddm_amd.models import SEED_LIMIT, MultiScaleGaussianDiffusion, noise_stream_id, vary_seeds

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the stream-id layout -------------------------------------------------------------------------------------------------
def test_stream_ids_are_distinct_and_laid_out_per_scale():
    ids = {}
    for s in range(6):
        ids[(s, "init", 0)] = noise_stream_id(s, "init")
        ids[(s, "renoise", 0)] = noise_stream_id(s, "renoise")
        for i in range(1100):
            ids[(s, "step", i)] = noise_stream_id(s, "step", i)
    assert len(set(ids.values())) == len(ids)
    assert noise_stream_id(0, "init") == 0 and noise_stream_id(0, "renoise") == 1 and noise_stream_id(0, "step", 0) == 2
    assert noise_stream_id(3, "step", 5) == (3 << 32) | 7
    assert all(0 <= v < 2 ** 64 for v in ids.values())
    with pytest.raises(ValueError):
        noise_stream_id(0, "init", 1)                           # only steps have a position
    with pytest.raises(ValueError):
        noise_stream_id(0, "step", 2 ** 32)                     # would run into the next scale's ids
    with pytest.raises(KeyError):
        noise_stream_id(0, "other")


# ---- vary_seeds -----------------------------------------------------------------------------------------------------------
def test_vary_seeds():
    seeds = [17, 17, 17, 17]
    rows = vary_seeds(seeds, 3, 5)
    assert rows == vary_seeds(list(seeds), 3, 5)                # deterministic
    assert len(rows) == 5 and all(len(r) == 4 for r in rows)
    assert rows[0] == rows[1] == rows[2] == seeds               # below from_scale: unchanged
    assert rows[3] == rows[4] and len(set(rows[3])) == 4        # distinct per b although the inputs are equal
    assert all(0 <= v < SEED_LIMIT for v in rows[3])
    assert not set(rows[3]) & set(seeds)
    # the derived seed depends on the given seed and on the position
    other = vary_seeds([17, 18, 17, 17], 3, 5)
    assert other[3][0] == rows[3][0] and other[3][1] != rows[3][1] and other[3][2] == rows[3][2]
    assert vary_seeds(seeds, 0, 2)[0] == rows[3] and vary_seeds(seeds, 5, 5) == [seeds] * 5
    big = vary_seeds(list(range(4096)), 0, 1)[0] + vary_seeds([SEED_LIMIT - 1] * 64, 0, 1)[0]
    assert all(0 <= v < SEED_LIMIT for v in big) and len(set(big[:4096])) == 4096 and len(set(big[4096:])) == 64
    for bad in ([-1], [SEED_LIMIT], [1.5], [True]):
        with pytest.raises(ValueError):
            vary_seeds(bad, 0, 2)
    with pytest.raises(ValueError):
        vary_seeds(seeds, 6, 5)


# ---- the rank slice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,world", [(4, 2), (7, 3), (5, 4), (16, 8), (3, 1), (9, 8)])
def test_shard_seeds_cover_the_batch_once(B, world, monkeypatch):
    seeds = [1000 + 3 * b for b in range(B)]
    monkeypatch.setattr(sdist, "world_size", lambda: world)
    got, sizes = [], sdist.shard_sizes(B, world)
    for r in range(world):
        monkeypatch.setattr(sdist, "rank", lambda r=r: r)
        part = sdist.shard_seeds(seeds)
        assert len(part) == sizes[r] == sdist.local_batch(B)
        got += part
    assert got == seeds                                         # every sample exactly once, in gather_batch's order


def test_shard_seeds_single_process():
    assert sdist.shard_seeds([5, 6, 7]) == [5, 6, 7]


# ---- sample_seeds on the diffusion -----------------------------------------------------------------------------------------
def _diffusion():
    sizes = [(16, 12), (24, 18), (32, 24)]                      # (W, H) as create_img_scales gives them
    return MultiScaleGaussianDiffusion(None, n_scales=3, scale_factor=1.4, image_sizes=sizes, timesteps=10,
                                       scale_losses=[0.5, 0.4], train_full_t=True)


def test_sample_seeds_forms_and_errors():
    d = _diffusion()
    assert d.sample_seeds is None and d._seeds_for(0, 4) is None
    d.sample_seeds = [5, 6, 7]
    assert d._seeds_for(0, 3) == d._seeds_for(2, 3) == [5, 6, 7]
    d.sample_seeds = torch.tensor([5, 6, 7])
    assert d._seeds_for(1, 3) == [5, 6, 7]
    d.sample_seeds = [[1, 2], [3, 4], [5, 6]]
    assert [d._seeds_for(s, 2) for s in range(3)] == [[1, 2], [3, 4], [5, 6]]
    d.sample_seeds = vary_seeds([9, 9], 1, 3)
    assert d._seeds_for(0, 2) == [9, 9] and len(set(d._seeds_for(2, 2))) == 2
    d.sample_seeds = [5, 6, 7]
    with pytest.raises(ValueError):
        d._seeds_for(0, 4)                                      # count does not match the batch
    with pytest.raises(ValueError):
        d._draw("init", (2, 3, 8, 8), 0, 0, "cpu")              # ... raised before anything is drawn
    d.sample_seeds = [[1, 2], [3, 4]]
    with pytest.raises(ValueError):
        d._seeds_for(0, 2)                                      # rows do not match the scales
    for bad in ([-1, 2], [1, SEED_LIMIT], [1, 2.5]):
        d.sample_seeds = bad
        with pytest.raises(ValueError):
            d._seeds_for(0, 2)
    d.sample_seeds = [0, SEED_LIMIT - 1]
    assert d._seeds_for(0, 2) == [0, SEED_LIMIT - 1]
    d.noise_fn = lambda kind, shape, s, t, device: torch.zeros(shape)
    with pytest.raises(ValueError):
        d._seeds_for(0, 2)                                      # two noise sources
    with pytest.raises(ValueError):
        d._run_steps(torch.zeros(2, 3, 8, 8), 0, [1, 0])
    d.sample_seeds = None
    assert d._seeds_for(0, 2) is None                           # noise_fn alone stays what it was
    assert d._draw("init", (2, 3, 8, 8), 0, 0, "cpu").shape == (2, 3, 8, 8)


def test_driver_seed_lists():
    """MultiscaleTrainer._local_seeds: the global list checked, varied on GLOBAL positions, then cut to the rank."""
    from sinddm_amd.trainer import MultiscaleTrainer

    class T:
        n_scales = 4
    f = lambda *a, **k: MultiscaleTrainer._local_seeds(T(), *a, **k)
    assert f(None, None, 4, sharded=True) is None
    assert f([1, 2, 3, 4], None, 4, sharded=True) == [1, 2, 3, 4]
    assert f([7, 7], 2, 2, sharded=False) == vary_seeds([7, 7], 2, 4)
    for args in (([1, 2, 3], None, 4), (None, 2, 4), ([1, -2], None, 2)):
        with pytest.raises(ValueError):
            f(*args, sharded=True)


# ---- the command line -----------------------------------------------------------------------------------------------------
def test_cli_seed_flags(capsys):
    sys.path.insert(0, REPO)
    try:
        import main as cli
    finally:
        sys.path.remove(REPO)
    a = cli.parse_args(["--mode", "sample", "--sample_batch_size", "3", "--seeds", "4", "5", "6"])
    assert a.seeds == [4, 5, 6] and a.vary_from_scale is None
    a = cli.parse_args(["--mode", "sample", "--sample_batch_size", "3", "--seed_base", "40", "--vary_from_scale", "2"])
    assert a.seeds == [40, 41, 42] and a.vary_from_scale == 2
    a = cli.parse_args(["--mode", "sample"])
    assert a.seeds is None and a.seed_base is None and a.vary_from_scale is None
    for argv in (["--sample_batch_size", "4", "--seeds", "1", "2", "3"],                  # wrong length
                 ["--sample_batch_size", "2", "--seeds", "1", "2", "--seed_base", "5"],   # both
                 ["--sample_batch_size", "2", "--vary_from_scale", "1"],                  # variations of nothing
                 ["--sample_batch_size", "2", "--seeds", "1", "-2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    capsys.readouterr()


# ---- the C ABI: validation before any device work ---------------------------------------------------------------------------
def test_abi_validation_without_a_device():
    lib = _lib.load()
    assert {"sinddm_normal_fill_samples", "sinddm_sample_chain_seeds"} <= set(_lib.ABI_SYMBOLS)
    assert lib.sinddm_abi_version() == 3
    # (fake non-null device pointers: validation returns before anything is enqueued or dereferenced)
    assert lib.sinddm_normal_fill_samples(None, 1, 16, 256, 0, None) == -1
    assert lib.sinddm_normal_fill_samples(256, 1, 16, None, 0, None) == -1
    assert lib.sinddm_normal_fill_samples(256, 0, 16, 256, 0, None) == -1
    assert lib.sinddm_normal_fill_samples(256, -2, 16, 256, 0, None) == -1
    assert lib.sinddm_normal_fill_samples(256, 1, 0, 256, 0, None) == -1
    assert lib.sinddm_normal_fill_samples(256, 1, -5, 256, 0, None) == -1
    assert lib.sinddm_normal_fill_samples(256, 1, 16, 260, 0, None) == -1               # seeds not 8-byte aligned
    one = C.cast(C.pointer(_lib.StepCoefs()), C.POINTER(_lib.StepCoefs))
    tl = (C.c_int * 1)(0)
    flag = C.c_int(7)

    def chain(seeds, x=256):
        return lib.sinddm_sample_chain_seeds(256, 256, x, 256, 256, None, one, tl, 1, 0.0, 1, 0, 160, 1, 8, 8, 256, 0, None, None,
                                             C.byref(flag), None, 0, 0, None, seeds)

    assert chain(260) == -1 and chain(257) == -1                # SINDDM_E_BADARG: not 8-byte aligned
    assert chain(264, x=None) == -1
    assert chain(264) == -3                                     # accepted: the (empty) workspace is what fails next
    assert chain(None) == -3                                    # NULL: sinddm_sample_chain_keep itself
    assert lib.sinddm_sample_chain_seeds(256, 256, 256, 256, 256, None, one, tl, 1, 0.0, 1, 0, 160, 1, 8, 8, 256, 0, None, None,
                                         C.byref(flag), None, 3, 0, None, 264) == -1     # a halo below 16, as before
    assert flag.value == 7
