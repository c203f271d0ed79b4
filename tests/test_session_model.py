"""The committed editing sessions (tests/session_model.py SESSION_SPECS) are worth running: this runs them through the model
alone, on the CPU, and asserts what they reach — so that a green tests/test_gpu_sessions.py cannot be a hollow one.  The
conditions are fixed; the seeds were searched for them.  The summary each test prints lists, per session, the count of each step
kind, the no-op and misfit share and the steps at which each condition is met."""
import numpy as np
import pytest

import session_model as sm
from tdt4230_project_raytracing_amd import rt


@pytest.fixture(scope="module")
def summaries(oracle):
    out = {}
    for name in sm.SESSION_SPECS:
        s = sm.session(name, oracle)
        out[name] = (s, sm.summarise(s, oracle))
        print(sm.summary_text(out[name][1]))
    return out


def test_every_kind_occurs(summaries):
    total = {}
    for _, r in summaries.values():
        for k, n in r["kinds"].items():
            total[k] = total.get(k, 0) + n
    print("all sessions:", " ".join(f"{k}:{total.get(k, 0)}" for k in sm.ALL_KINDS))
    assert all(total.get(k, 0) >= 2 for k in sm.EDIT_KINDS), total
    assert all(total.get(k, 0) >= 1 for k in sm.READ_KINDS), total
    # the three single-device sessions alone hold every kind, and the depth-6 one only kinds whose models stay fast there
    single = set().union(*[summaries[n][1]["kinds"] for n in ("d4", "d5a", "d5b")])
    assert single == set(sm.ALL_KINDS), set(sm.ALL_KINDS) - single
    assert set(summaries["d6"][1]["kinds"]) <= set(sm.FAST_KINDS)


def test_steps_mostly_change_the_tree_and_some_do_not_fit(summaries):
    for name, (_, r) in summaries.items():
        assert (len(r["noops"]) + len(r["misfits"])) * 4 <= r["edits"], sm.summary_text(r)
        assert r["nonempty"] * 5 >= 4 * r["steps"], sm.summary_text(r)
    assert any(r["misfits"] and r["misfit_then_fit"] for _, r in summaries.values())
    for name in ("d4", "d5a", "two_members", "rendered_d5"):                                    # (more than one: on a bare context, in a scene, on two members)
        r = summaries[name][1]
        assert r["misfits"] and r["misfit_then_fit"] and r["misfit_then_fit"][0] > r["misfits"][0], sm.summary_text(r)


def test_a_session_passes_through_the_empty_tree_and_comes_back(summaries):
    through = [n for n, (_, r) in summaries.items() if r["empty"] and r["back_from_empty"] and r["back_from_empty"][-1] > r["empty"][0]]
    print("through the empty tree:", through)
    assert through
    assert "rendered" in through                                      # (one of them renders it)


def test_a_fill_or_close_merges_leaves(summaries):
    """tree_model.build_cells of the tree after the step holds more LEAFs above the finest level than before it."""
    merging = {n: r["merging_fill_or_close"] for n, (_, r) in summaries.items() if r["merging_fill_or_close"]}
    print("fill / close steps that merge subtrees into leaves:", merging)
    assert merging


def test_point_edits_are_followed_by_unit_edits_and_by_compacts(summaries):
    on_dead = {n: r["edit_on_point_edited_tree"] for n, (_, r) in summaries.items() if r["edit_on_point_edited_tree"]}
    lowers = {n: r["compact_lowers"] for n, (_, r) in summaries.items() if r["compact_lowers"]}
    print("unit edits on a tree left by point edits:", on_dead)
    print("compacts that lower the cell count:", lowers)
    assert on_dead and lowers
    for name in ("two_members", "rendered", "rendered_d5"):
        r = summaries[name][1]
        assert r["kinds"].get("points", 0) >= 1 and r["kinds"].get("compact", 0) >= 1 and r["compact_lowers"], sm.summary_text(r)


def test_the_depth_6_tree_crosses_the_bit_volume_boundaries(summaries):
    """Its bounding box crosses a 32-voxel word boundary and an 8 x 8 tile boundary of the bit-volume layout on every axis."""
    s, _ = summaries["d6"]
    lo, hi = s["V0"][:, :3].min(0), s["V0"][:, :3].max(0)
    assert (lo < 32).all() and (hi >= 32).all() and (lo // 8 != hi // 8).all()
    assert len(s["V0"]) < 0.01 * 64 ** 3                              # sparse


def test_the_rendered_depth_5_session_leaves_its_specialised_build(summaries):
    """A step after which the whole-depth table no longer serves the tree, seen by a render (they follow every second step), and a
    later one after which it does again."""
    s, r = summaries["rendered_d5"]
    m = sm.model_of(s)
    assert sm.whole_depth_table_fits(m.cells, m.depth)
    assert r["table_flips"] and r["table_flips"][0] % 2 == 1, sm.summary_text(r)
    assert len(r["table_flips"]) >= 2


def test_a_session_prints_in_a_form_that_replays(oracle):
    """format_session's text evaluates to steps that give the same trees again."""
    s = sm.session("d4", oracle)
    text = sm.format_session(s, upto=5)
    assert "seed" in text and "depth" in text
    steps = eval(text[text.index("steps = ") + 8:], {})               # noqa: S307 (the test's own text)
    V0 = np.array(eval(text.split("\n")[1][5:], {}), np.int32)        # noqa: S307
    assert len(steps) == 6 and np.array_equal(V0, s["V0"])
    a, b = sm.Model(V0, s["depth"], s["capacity"], s["floats"], s["ints"], oracle), sm.model_of(s, oracle)
    for mine, theirs in zip(steps, s["steps"]):
        x, y = a.step(mine), b.step(theirs)
        assert x.status == y.status and np.array_equal(x.V, y.V) and np.array_equal(x.cells, y.cells) and x.counter == y.counter
    V = sm.sort_vox(V0)
    for step in steps:
        if step[0] != "points":
            V = sm.apply(V, s["depth"], step)                         # (apply takes the printed form too)


def test_apply_restates_nothing():
    """Every list kind is the unit's own model composed with apply_op: spot checks against direct calls."""
    import fill_model
    import morph_model
    from test_gpu_region_edit import expected_region
    rng = np.random.default_rng(5)
    V = sm.initial_tree(rng, 4, 254)
    g = [("sphere", [5, 5, 5], 3)]
    assert np.array_equal(sm.apply(V, 4, ("region", dict(op=rt.REGION_SET, regions=g, material=9))), expected_region(V, rt.REGION_SET, sm.regions_of(g), 9, 4))
    assert np.array_equal(sm.apply(V, 4, ("morph", dict(op=rt.MORPH_SHELL, radius=1, connectivity=26, material=None, border=0, regions=None))),
                          morph_model.morph(V, 4, rt.MORPH_SHELL, 1, 26))
    assert np.array_equal(sm.apply(V, 4, ("fill", dict(connectivity=6, material=None, regions=None))), fill_model.filled(V, 4))
    assert np.array_equal(sm.apply(V, 4, ("compact", {})), V) and np.array_equal(sm.apply(V, 4, ("extract", {})), V)
    with pytest.raises(ValueError):
        sm.apply(V, 4, ("points", dict(delta=np.zeros((1, 8), np.float32))))
    raw = np.array([[1, 1, 1, 5], [16, 0, 0, 9], [1, 1, 1, 7]], np.int32)
    assert sm.list_meaning(raw, 4).tolist() == [[1, 1, 1, 7]]
