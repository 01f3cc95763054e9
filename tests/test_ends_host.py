"""Host-only pieces of the inference plans' ends: the two pass schedules, the plan cache and the merged validators."""
import types

import pytest

from esrganplus_amd import engine as E
from esrganplus_amd import functional as F


@pytest.mark.parametrize('slots', [8, 4, 2, 1])
def test_x8_passes_cover_the_eight_transforms_once_in_order(slots):
    passes = E.x8_passes(slots)
    assert [k for k0, _, _, _ in passes for k in range(k0, k0 + slots)] == list(range(8))
    assert [acc for _, _, acc, _ in passes] == [0] + [1] * (len(passes) - 1)
    assert [scale for _, _, _, scale in passes] == [1.0] * (len(passes) - 1) + [0.125]
    for k0, i, _, _ in passes:
        assert i == (0 if k0 < 4 else -1)
        assert ['a', 'b'][i] == ('a' if k0 < 4 else 'b') and ['a'][i] == 'a'      # two plans: the last; one plan: that one


def test_tile_passes():
    assert list(E.tile_passes(12, 5)) == [0, 5, 10]
    assert list(E.tile_passes(12, 12)) == [0]


def _holder():
    return types.SimpleNamespace(_plans={}, max_cached_plans=2)


def test_cached_plan_hit_returns_the_same_object_without_building():
    mod, built = _holder(), []

    def build():
        built.append(1)
        return object()
    a = F._cached_plan(mod, ('k', 1), build)
    assert F._cached_plan(mod, ('k', 1), build) is a and built == [1] and mod._plans == {('k', 1): a}


def test_cached_plan_empties_a_full_cache_before_it_builds():
    mod, seen = _holder(), []
    F._cached_plan(mod, 'a', object)
    F._cached_plan(mod, 'b', object)
    assert list(mod._plans) == ['a', 'b']

    def build():
        seen.append(dict(mod._plans))
        return object()
    c = F._cached_plan(mod, 'c', build)
    assert seen == [{}] and mod._plans == {'c': c}


def test_cached_plan_a_build_that_raises_leaves_the_cache_as_it_was():
    mod = _holder()
    a = F._cached_plan(mod, 'a', object)

    def build():
        raise RuntimeError('refused')
    with pytest.raises(RuntimeError, match='refused'):
        F._cached_plan(mod, 'b', build)
    assert mod._plans == {'a': a}


BAD = [(dict(tile=0), 'tile of a tiled forward must be an int >= 1, got 0'),
       (dict(pad=-1), 'pad of a tiled forward must be an int >= 0, got -1'),
       (dict(tiles_per_pass=True), 'tiles_per_pass of a tiled forward must be an int >= 1, got True'),
       (dict(windows_per_pass=1.5), 'windows_per_pass of a tiled forward must be an int >= 1, got 1.5')]


@pytest.mark.parametrize('bad,message', BAD)
def test_merged_validators_keep_their_messages(bad, message):
    per_image = dict(tile=8, pad=2, tiles_per_pass=5)
    image_set = dict(tile=8, pad=2, windows_per_pass=5)
    raised = []
    for fn, args in ((lambda **kw: F._tiled_args(2, 20, 27, **kw), per_image),
                     (lambda **kw: F.tiled_many_passes([(9, 20), (13, 13)], **kw), image_set)):
        if set(bad) <= set(args):
            with pytest.raises(ValueError) as e:
                fn(**dict(args, **bad))
            raised.append(str(e.value))
    assert raised and all(m == message for m in raised), raised


def test_merged_validators_accept_what_they_accepted():
    import numpy as np
    assert F._tiled_args(2, 20, 27, np.int64(8), 2, None) == (8, 2, 8)        # default P = 16 // B, an index type as tile
    assert F._tiled_args(1, 20, 27, 64, 40, 5) == (27, 27, 1)                 # cut down to the image
    assert F._tiled_many_ints(8, 0, 16) == (8, 0, 16)
