"""CPU-only checks of GPSO_OPT_SURVIVOR_TILE at the C-ABI boundary: the option's number, its documented values and its default
are the same in the header, in the library's sources and in the ctypes binding; without a context the entry point refuses.  (Its
validation on a live context, and what it does, are tests/test_gpu_screen_narrow.py's.)  And the pure host model that says up to
how many survivors the narrow tile runs (csrc/screen.hpp: survivor_narrow_max, exported as gpso_survivor_narrow_max_host)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from pygpso_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_option_number_and_its_values_agree_everywhere():
    from pygpso_amd import _lib
    from pygpso_amd.engine import HipGPEngine

    header = _read("include", "gpso_hip.h")
    assert re.search(r"#define GPSO_OPT_SURVIVOR_TILE 16\b", header)
    assert _lib.OPT_SURVIVOR_TILE == 16
    numbers = [int(v) for v in re.findall(r"#define GPSO_OPT_[A-Z0-9_]+ (\d+)", header)]
    assert len(numbers) == len(set(numbers)), "two options share a number"
    assert callable(HipGPEngine.set_survivor_tile)
    # the validation the C-ABI applies: 0, 1, 2 and nothing else
    api = _read("pygpso_amd", "csrc", "api.hip")
    case = api[api.index("case GPSO_OPT_SURVIVOR_TILE:"):]
    case = case[:case.index("return GPSO_OK;")]
    assert "value < 0 || value > 2" in case and "GPSO_E_ARG" in case and "survivor_tile = value" in case


def test_the_default_is_narrow_for_the_survivors_and_the_wide_arm_is_a_build_flag():
    ctx = _read("pygpso_amd", "csrc", "context.hpp")
    m = re.search(r"#ifndef GPSO_SURVIVOR_TILE_DEFAULT\s*\n#define GPSO_SURVIVOR_TILE_DEFAULT (\d+)", ctx)
    assert m and int(m.group(1)) == 0
    core = _read("pygpso_amd", "csrc", "engine_core.hpp")
    assert "int survivor_tile = GPSO_SURVIVOR_TILE_DEFAULT;" in core


def test_without_a_context_the_entry_points_refuse(lib):
    from pygpso_amd import _lib

    assert lib.gpso_set_option(None, _lib.OPT_SURVIVOR_TILE, 0) == _lib.E_ARG
    assert lib.gpso_last_count(None, 9) == -1


def test_the_threshold_model_at_the_bench_shapes_and_its_monotonicity(lib):
    """A narrow k-step takes 0.52 of a wide one; a launch lasts as long as its heaviest row block's chain (8 nbi steps) or the
    chip's share of all steps (tiles x 4 nbi (nbi + 1) / CUs), whichever is longer.  C3: N = 2048 is 8 row blocks, a room of
    8 192 rows on 256 CUs -- narrow up to 109 narrow tiles (0.52 x 1.125 x 109 = 63.8 < 64); the C4 share: 32 row blocks, a room
    of 2 048 rows -- up to 29 (0.52 x 16.5 x 29 = 248.8 < 256)."""
    f = lib.gpso_survivor_narrow_max_host
    assert f(8, 256, 8192) == 109 * 64 == 6976
    assert f(32, 256, 2048) == 29 * 64 == 1856
    # the bench seeds' counts (28 .. 920 at C3, 1 748 at C4) are far on the narrow side
    assert f(8, 256, 8192) > 920 and f(32, 256, 2048) > 1748
    # small posteriors never reach the crossover inside their room: one launch, narrow
    assert f(3, 256, 1024) == 1024 and f(1, 256, 256) == 256
    # the restated model
    def model(nbi, ncu, cap):
        chain, per_tile, best = 8.0 * nbi, 4.0 * nbi * (nbi + 1.0) / ncu, 0
        for c in range(64, cap + 1, 64):
            narrow = 0.52 * max(chain, per_tile * (c // 64))
            wide = max(chain, per_tile * ((c + 255) // 256))
            if not narrow < wide:
                break
            best = c
        return best
    for nbi in (1, 2, 3, 8, 16, 32, 64):
        for ncu in (64, 256, 304):
            caps = [256 * k for k in (1, 2, 8, 32, 85, 128)]
            got = [f(nbi, ncu, cap) for cap in caps]
            assert got == [model(nbi, ncu, cap) for cap in caps]
            assert all(g % 64 == 0 and 0 <= g <= cap for g, cap in zip(got, caps))
            assert got == sorted(got)  # (more room never lowers it)
            # monotone in the count: the narrow side is a prefix -- every count up to the answer is narrow in the model, none above
            top = f(nbi, ncu, 1 << 20)
            assert all(f(nbi, ncu, c) == min(c, top) for c in range(64, 4096 + 1, 64))
    assert f(0, 256, 1024) < 0 and f(8, 0, 1024) < 0 and f(8, 256, -1) < 0


def test_the_narrow_workgroup_fits_the_lds_at_every_shape_the_family_takes():
    """leaf_bf16_lds_bytes (kernels.hpp) restated for the fp16 contraction: two buffers of L^-1 pieces, three X buffers, and per
    wave ct halves of a k-step's X fragments.  One narrow workgroup fits a CU's 160 KB wherever the wide one does, two do not."""

    def lds(dp4, nw, ct):
        xfrag = (dp4 + 8) // 8 * 4096
        return 2 * 2 * 16 * 64 * 16 + 3 * (xfrag + 64 * 4 + 256) + nw * (xfrag // 2 * ct)

    for d_pad in (12, 20, 40, 48):
        wide, narrow = lds(d_pad // 4, 8, 2), lds(d_pad // 4, 4, 1)
        assert narrow < wide <= 160 * 1024 < 2 * narrow
    assert lds(3, 4, 1) == 87552 and lds(10, 4, 1) == 108032
