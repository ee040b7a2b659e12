"""AbsorptionRun._plan: the launches of the constant sources, their batch policy and the collectives of every rank,
decided before any engine call (built here for ranks of a world of 2 from a stand-in comm, no process group)."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host import _write_model                 # noqa: E402
from soc_amd import synth                          # noqa: E402
from soc_amd.asoc import AbsorptionRun              # noqa: E402
from soc_amd.ini import User                        # noqa: E402

R = AbsorptionRun
# (grid, ini lines) -> the policy of each source block (PS, BG, DE), as the conditions of the per-block loops picked them
CONFIGS = {
    "tabs_only": ("octree", "noabsorbed\n", [R.ONE_BATCH] * 3),
    "tabs_only_cartesian": ("cartesian", "noabsorbed\n", [R.ONE_BATCH] * 3),
    "absorbed_hierarchy": ("octree", "", [R.FREQ_GROUPS] * 3),
    "absorbed_cartesian": ("cartesian", "", [R.LAUNCH_GROUPS] * 3),
    "saveint_hierarchy": ("octree", "saveint 1 {d}/int.bin\n", [R.SEQUENTIAL] * 3),
    "saveint_cartesian": ("cartesian", "saveint 1 {d}/int.bin\n", [R.SEQUENTIAL] * 3),
    "roisave_cartesian": ("cartesian", "roi 2 4 2 4 2 3\nroisave {d}/roi.save 1\nroinside 2\n", [R.SEQUENTIAL] * 3),
    "roisave_tabs_only": ("octree", "noabsorbed\nroi 2 4 2 4 2 3\nroisave {d}/roi.save 1\nroinside 2\n", [R.SEQUENTIAL] * 3),
    "hpbg_hierarchy": ("octree", "hpbg {d}/sky.bin 2.0 1\n", [R.SEQUENTIAL] * 3),
    "hpbg_cartesian": ("cartesian", "hpbg {d}/sky.bin 2.0 1\n", [R.LAUNCH_GROUPS] * 3),
    "no_iterations": ("octree", "iterations 0\n", []),
    "one_rank_per_launch_item": ("octree", "global 64\nbgpackets 0\n", [R.FREQ_GROUPS] * 2),
}


def _model(d, name):
    grid, extra, _ = CONFIGS[name]
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9) if grid == "octree" else synth.cartesian_cloud(6, seed=9)
    sky = np.random.default_rng(3).lognormal(0, 1, (3, 49152)).astype(np.float32) * 1e-13
    sky[1] = 0.0                                                   # an empty sky at one frequency: the background sends nothing there
    sky.tofile(os.path.join(d, "sky.bin"))
    return _write_model(d, cloud, with_ps=True, with_diffuse=True, extra=extra.format(d=d))


def _plan(ini, rank=0, world=1, shard="items"):
    comm = types.SimpleNamespace(rank=rank, world=world) if world > 1 else None
    run = AbsorptionRun(User(ini), None, comm, verbose=0, shard=shard)
    run.ROI_LOAD = None
    return run, run._plan(not run.U.NOABSORBED, 1)


def _shape(segments):
    """everything of a plan but this rank's work items: the same on every rank"""
    return [(policy, name, [(f, [m[0] for m in launches], summed) for f, launches, summed in steps]) for policy, name, steps in segments]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_policy_of_every_block(name, tmp_path):
    _, (segments, owner) = _plan(_model(str(tmp_path), name))
    blocks = {}
    for policy, _, steps in segments:
        for _, launches, summed in steps:
            assert not summed                                      # one rank: nothing to sum
            for II, L, first, count in launches:
                assert (first, count) == (0, L["GLOBAL"])
                assert blocks.setdefault(II, policy) == policy
    assert [blocks[II] for II in sorted(blocks)] == CONFIGS[name][2] and owner is None
    if blocks and blocks[min(blocks)] in (R.ONE_BATCH, R.FREQ_GROUPS):
        assert len(segments) == 1 and segments[0][1] == "all source blocks"     # TABS read once
    elif blocks:
        assert [name for _, name, _ in segments] == ["PS", "BG", "DE"]             # TABS read per block
    order = [(II, f) for _, _, steps in segments for f, launches, _ in steps for II, _, _, _ in launches]
    if segments and segments[0][0] == R.FREQ_GROUPS:
        assert order == sorted(order, key=lambda x: (x[1], x[0]))                 # frequency outside
    else:
        assert order == sorted(order)                                              # source block outside


@pytest.mark.parametrize("shard", ["items", "launches"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_two_ranks_cover_every_work_item_once_and_enter_the_same_collectives(name, shard, tmp_path):
    ini = _model(str(tmp_path), name)
    run, (single, _) = _plan(ini)
    plans = [_plan(ini, rank, 2, shard)[1] for rank in (0, 1)]
    assert _shape(plans[0][0]) == _shape(plans[1][0])
    assert plans[0][1] == plans[1][1]
    items = {}
    for segments, _ in plans:
        for _, _, steps in segments:
            for f, launches, _ in steps:
                for II, L, first, count in launches:
                    items.setdefault((II, f), []).extend(range(first, first + count))
    want = {(II, f): list(range(L["GLOBAL"])) for _, _, steps in single for f, launches, _ in steps for II, L, _, _ in launches}
    assert {k: sorted(v) for k, v in items.items()} == want
    owner = plans[0][1]
    for _, _, steps in plans[0][0]:
        for f, launches, summed in steps:
            if owner is not None or not (run.with_int or run.U.WITH_ROI_SAVE):
                assert not summed                                  # a frequency of one owner / TABS only: no collective per launch
            else:
                # the tallies of every launch that sends something are summed over the ranks, also where a rank has no work in it
                assert summed == (f != 1 or any(II != 1 or len(run.HPBG) == 0 for II, _, _, _ in launches))
    if name == "one_rank_per_launch_item" and shard == "items":
        idle = [s for s in plans[1][0][0][2] if all(m[3] == 0 for m in s[1])]
        assert idle and all(summed for _, _, summed in idle)      # rank 1 has no work item and still enters the collectives
