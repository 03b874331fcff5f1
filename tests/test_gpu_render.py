"""GPU: wk_render / wk_render_device / wk_render_states against tests/renderref.py, byte for byte.

The reference frames are built from what the public getters return -- get_state's records,
body_view's floor polygons (the flat floor or the 10 rough segments), prop_view's vertices -- so the
kernel's own reading of the records, the terrain and the props block is what is under test.  Every
equality case first asserts on the REFERENCE frame that at least 1 % of its pixels are lit and that
it holds the colours the case is about (two black frames cannot pass), then that the kernel's
bytes are the same.  The windows: 128 x 96 at scale 0.5 following the torso from y = 739, which puts
the floor's top edge (y = 900) on the centres of row 80 -- on a pixel border a one-pixel line lights
nothing, the rule's width is strict -- and shows the walker above it.
Every case prints its figures (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import renderref as R

pytestmark = pytest.mark.gpu

SEED = 20250905
F = np.float32
WIN = dict(width=128, height=96, follow=1, ox=0.0, oy=739.0)
STATIC = dict(shape="Square", material="Metal", is_static=True, cx=215.0, cy=880.0, size=30.0)
DYNAMIC = dict(shape="Hexagon", smooth=1, material="Wood", is_static=False, cx=40.0, cy=850.0, size=24.0, ay=980.0)


def _floor(eng, e, rough):
    views = [eng.body_view(e, 5 + k) for k in range(10 if rough else 1)]
    assert all(v.n_vertices == 4 and v.is_static for v in views)
    return [np.array(v.vertices, F)[:4] for v in views]


def _props(eng, e, scene):
    return [(eng.prop_view(e, k).vertex_array(), bool(p.is_static), int(p.material)) for k, p in enumerate(scene)]


def reference(eng, envs, mats, kw, states=None, rough=False, scene=()):
    a = R.args(**kw)
    st = eng.get_state() if states is None else np.asarray(states, F).reshape(len(envs), -1)
    return np.stack([R.render_view(st[e] if states is None else st[i], int(mats[e]), a, _floor(eng, e, rough),
                                   _props(eng, e, scene)) for i, e in enumerate(envs)])


def check(eng, envs, mats, kw, colours, joint="as asked", states=None, rough=False, scene=(), what=""):
    """reference, the black-frame condition on it, then byte equality; returns the frames.  joint:
    whether every reference frame must show a joint colour -- by default exactly when joints are
    drawn; None where the case's scale leaves a 3-unit square under a pixel"""
    ref = reference(eng, envs, mats, kw, states, rough, scene)
    joint = bool(R.args(**kw)["joints"]) if joint == "as asked" else joint
    for i, e in enumerate(envs):
        R.assert_shows(ref[i], list(colours) + [R.MATERIAL_RGB[int(mats[e])]], (what, i, e))
        assert joint is None or R.has_joint_colour(ref[i]) == joint, (what, i, e)
    got = eng.render(envs, **kw) if states is None else eng.render_states(states, envs, **kw)
    diff = int((got != ref).any(axis=-1).sum())
    print(f"{what}: {len(envs)} views {ref.shape[2]} x {ref.shape[1]}, lit {R.lit_fraction(ref):.4f}, "
          f"differing pixels {diff}")
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert got.tobytes() == ref.tobytes(), (what, diff)
    return got


@pytest.fixture(scope="module")
def flat(wk):
    """8 walkers on the flat floor at their own start offsets, stepped 30 env-steps by test order"""
    eng = wk.Engine(8, seed=SEED, RandomizeStart=1, Horizon=8, Minibatch=8)
    yield eng
    eng.close()


CARPET = [0] * 70


def test_fresh_flat_floor(flat):
    check(flat, [0, 1, 2, 3], CARPET, WIN, [R.WHITE], what="fresh")
    # the fixed window: no follow, the walkers start between x = 125 and 325
    # (at scale 0.25 a joint's 3-unit square is under a pixel: drawn without joints, and asserted so)
    check(flat, [0, 5], CARPET, dict(width=128, height=96, scale=0.25, ox=0.0, oy=610.0, joints=0), [R.WHITE],
          joint=False, what="fixed window")


def test_after_30_sampled_steps(flat):
    flat.step(None, 30)
    st = flat.get_state()
    assert np.abs(st[:, R.ST_TORQUE:R.ST_TORQUE + 4]).max() > 0  # the joints are coloured by live torques
    check(flat, [0, 1, 2, 3, 4, 5, 6, 7], CARPET, WIN, [R.WHITE], what="after 30 steps")


@pytest.mark.parametrize("line_px", [1.0, 2.5])
def test_line_thickness(flat, line_px):
    check(flat, [1, 6], CARPET, dict(WIN, line_px=line_px), [R.WHITE], what=f"line_px {line_px}")


def test_marker_and_no_joints(flat):
    st = flat.get_state()
    mx = float(st[2, R.ST_POS]) + 40.0
    got = check(flat, [2], CARPET, dict(WIN, marker_x=mx), [R.WHITE, R.LIME], what="marker")
    assert R.has_colour(got[0], R.LIME)
    got = check(flat, [2, 3], CARPET, dict(WIN, joints=0), [R.WHITE], joint=False, what="joints off")
    assert not R.has_joint_colour(got)


@pytest.mark.parametrize("name,kw,colours,joint", [
    # a joint square is 3 world units: at the scale that fits the floor and a leg into 9 rows it is
    # under half a pixel and the leg's outline paints over it, so this case is about White and the material
    ("17x9", dict(width=17, height=9, scale=0.125, follow=1, ox=0.0, oy=836.5), [R.WHITE], None),
    # one pixel, its centre on the floor's top edge: White is all it can hold
    ("1x1", dict(width=1, height=1, scale=0.5, ox=100.0, oy=899.0), [R.WHITE], None),
    ("130x67", dict(width=130, height=67, scale=0.5, follow=1, ox=0.0, oy=789.0), [R.WHITE], True),
])
def test_sizes_off_the_tile(flat, name, kw, colours, joint):
    a = R.args(**kw)
    ref = reference(flat, [4], CARPET, kw)
    assert R.lit_fraction(ref) >= 0.01 and all(R.has_colour(ref, c) for c in colours), name
    if name != "1x1":
        assert R.has_colour(ref, R.GRAY), name
    if joint:
        assert R.has_joint_colour(ref)
    got = flat.render([4], **kw)
    print(f"{name}: lit {R.lit_fraction(ref):.4f}, differing pixels {int((got != ref).any(axis=-1).sum())}")
    assert got.shape == (1, a["height"], a["width"], 4) and got.tobytes() == ref.tobytes()


def test_70_views_repeated_and_unordered(flat):
    ids = np.random.default_rng(5).integers(0, flat.n, 70).tolist()
    assert len(set(ids)) < 70 and ids != sorted(ids)
    got = check(flat, ids, CARPET, WIN, [R.WHITE], what="70 views")
    first = {}
    for i, e in enumerate(ids):  # a repeated walker gives the same frame, wherever it stands in the list
        assert got[i].tobytes() == got[first.setdefault(e, i)].tobytes()


def test_materials_colour_the_walkers(wk, orc):
    n = 16
    eng = wk.Engine(n, seed=SEED, RandomizeMaterial=1)
    mats = [int(orc.env_material(SEED, e)) for e in range(n)]
    assert {R.MATERIAL_RGB[m] for m in mats} == {R.GRAY, R.CYAN}
    got = check(eng, list(range(n)), mats, WIN, [R.WHITE], what="RandomizeMaterial")
    assert any(R.has_colour(got[i], R.CYAN) for i in range(n)) and any(R.has_colour(got[i], R.GRAY) for i in range(n))
    # every colour of the table, through wk_set_materials
    mats = [0, 1, 2, 3, 4, 5, 6, 7] * 2
    eng.set_materials(mats)
    got = check(eng, [1, 3, 4, 6, 7], mats, WIN, [R.WHITE], what="set_materials")
    assert R.has_colour(got[2], R.SANDYBROWN) and R.has_colour(got[3], R.SLATEGRAY) and R.has_colour(got[0], R.CYAN)
    eng.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_rough_floor(wk, lanes):
    eng = wk.Engine(6, seed=SEED, RoughFloor=1, RandomizeStart=1, LanesPerWalker=lanes)
    kw = dict(WIN, oy=709.0)  # the terrain lies between y = 800 and y = 900
    check(eng, [0, 5], CARPET, kw, [R.WHITE], rough=True, what=f"rough fresh, lanes {lanes}")
    eng.step(None, 20)
    got = check(eng, [5, 0, 3], CARPET, kw, [R.WHITE], rough=True, what=f"rough after steps, lanes {lanes}")
    assert got[0].tobytes() != got[1].tobytes()  # per-walker terrain
    # the whole floor: 1100 world units in 138 columns
    # (at scale 0.125 a joint square is under half a pixel: drawn without joints, and asserted so)
    check(eng, [2], CARPET, dict(width=138, height=40, scale=0.125, ox=-52.0, oy=748.0, joints=0), [R.WHITE],
          rough=True, joint=False, what="rough whole floor")
    eng.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_lanes_per_walker(wk, lanes):
    eng = wk.Engine(5, seed=SEED, LanesPerWalker=lanes, RandomizeStart=1)
    check(eng, [4, 0], CARPET, WIN, [R.WHITE], what=f"lanes {lanes} fresh")
    eng.step(None, 30)
    check(eng, [0, 1, 2, 3, 4], CARPET, WIN, [R.WHITE], what=f"lanes {lanes} after steps")
    eng.close()


@pytest.mark.parametrize("rough", [0, 1])
def test_scene_props(wk, rough):
    eng = wk.Engine(4, seed=SEED, RoughFloor=rough)
    scene = [wk.make_prop(**STATIC), wk.make_prop(**DYNAMIC)]
    eng.set_scene(scene)
    eng.step(None, 12)
    kw = dict(WIN, oy=709.0) if rough else WIN
    got = check(eng, [0, 3], CARPET, kw, [R.WHITE, R.SANDYBROWN], rough=bool(rough), scene=scene,
                what=f"scene, rough {rough}")
    assert R.has_colour(got[0], R.SANDYBROWN)
    eng.close()


def _hand_built():
    """records for a window at scale 1 from (0, 879.5): world (x, y) is pixel (x, y - 879.5), the
    floor's top edge on the centres of row 20"""
    base = R.synthetic_record(x=70.0)
    base[R.ST_POS] = 70.0
    recs = {"base": base}
    r = base.copy()  # BODY: vertices on pixel centres and on the 64 x 16 tile borders
    r[40:50] = [63.5, 895.0, 64.0, 895.5, 64.5, 896.0, 80.5, 890.0, 64.0, 881.0]
    recs["centres and borders"] = r
    r = base.copy()  # LLL on tile corners exactly: (64, 16), (128, 16), (128, 32), (64, 32) in pixels
    r[0:12] = [64, 895.5, 96, 895.5, 128, 895.5, 128, 911.5, 96, 911.5, 64, 911.5]
    recs["tile corners"] = r
    r = base.copy()  # a body far outside the window
    r[60:72] += 1e5
    recs["far outside"] = r
    r = base.copy()
    r[20:32] = [1e30, 1e30, -1e30, 1e30, 1e30, -1e30, 3e30, 2e30, -1e30, -1e30, 1e30, 0.0]
    r[80] = 1e30
    recs["1e30"] = r
    r = base.copy()  # NaN and inf vertices: those segments vanish, the rest stays
    r[0], r[5] = np.nan, np.inf
    r[44] = -np.inf
    r[R.ST_TORQUE + 3] = np.nan
    recs["nan and inf"] = r
    r = base.copy()
    r[:100] = np.nan
    recs["all nan"] = r
    return recs


def test_render_states_hand_built(flat):
    kw = dict(width=130, height=40, scale=1.0, ox=0.0, oy=879.5)
    recs = _hand_built()
    names = list(recs)
    envs = [i % flat.n for i in range(len(names))]
    states = np.stack([recs[k] for k in names])
    before = flat.get_state()
    ref = reference(flat, envs, CARPET, kw, states=states)
    for i, k in enumerate(names):
        assert R.lit_fraction(ref[i]) >= 0.01 and R.has_colour(ref[i], R.WHITE), k
        assert R.has_colour(ref[i], R.GRAY) == (k != "all nan"), k
    got = flat.render_states(states, envs, **kw)
    for i, k in enumerate(names):
        d = int((got[i] != ref[i]).any(axis=-1).sum())
        print(f"hand-built {k}: lit {R.lit_fraction(ref[i]):.4f}, differing pixels {d}")
        assert got[i].tobytes() == ref[i].tobytes(), (k, d)
    # the segments of the broken bodies vanish and nothing else does: what the base frame shows of
    # the floor stays, and the broken frames only lose pixels of the walker
    base, nan = got[names.index("base")], got[names.index("nan and inf")]
    lost = (base != nan).any(axis=-1)
    assert 0 < lost.sum() < (base[..., :3] != 0).any(axis=-1).sum()
    assert (got[names.index("all nan")][20, :, :3] == 255).all()
    # a follow on a NaN torso draws a black frame and faults nothing
    r = recs["base"].copy()
    r[R.ST_POS] = np.nan
    black = flat.render_states(r[None], [0], **dict(kw, follow=1))
    assert (black[..., :3] == 0).all() and (black[..., 3] == 255).all()
    assert black.tobytes() == reference(flat, [0], CARPET, dict(kw, follow=1), states=r[None]).tobytes()
    # it only draws: the context's records are what they were, and the next step reports no fault
    assert flat.get_state().tobytes() == before.tobytes()
    assert not flat.step(None, 1)[3].any()


def test_render_device_into_a_guarded_tensor(flat):
    import torch
    kw, ids = dict(WIN, width=100, height=50, oy=819.0), [3, 0, 3]  # the floor on row 40's centres
    want = flat.render(ids, **kw)
    nbytes, guard = want.size, 64
    buf = torch.full((guard + nbytes + guard,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    shape = flat.render_device(buf.data_ptr() + guard, ids, **kw)
    flat.sync()
    host = buf.cpu().numpy()
    assert shape == want.shape
    assert (host[:guard] == 0xAB).all() and (host[guard + nbytes:] == 0xAB).all()
    assert host[guard:guard + nbytes].tobytes() == want.tobytes()
    R.assert_shows(want[0], [R.WHITE, R.GRAY], "render_device")
    with pytest.raises(Exception, match="aligned"):
        flat.render_device(buf.data_ptr() + guard + 1, ids, **kw)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == host).all()


def test_render_overwrites_every_byte(flat, wk):
    a = wk.render_args(**WIN)
    ids = np.array([1, 2], np.int32)
    img = np.full((2, a.height, a.width, 4), 0xAB, np.uint8)
    assert flat.lib.wk_render(flat.h, C.byref(a), ids.ctypes.data, 2, img.ctypes.data) == 0
    assert (img[..., 3] == 255).all()
    ref = reference(flat, [1, 2], CARPET, WIN)
    R.assert_shows(ref[0], [R.WHITE, R.GRAY], "prefilled")
    assert img.tobytes() == ref.tobytes()


def test_stream_order_after_an_asynchronous_rollout(flat):
    flat.rollout()            # no synchronise
    got = flat.render([0, 7], **WIN)
    after = flat.get_state()
    want = flat.render_states(after[[0, 7]], [0, 7], **WIN)
    R.assert_shows(want[0], [R.WHITE, R.GRAY], "stream order")
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == reference(flat, [0, 7], CARPET, WIN).tobytes()


def test_rendering_changes_nothing_of_a_training_run(wk):
    import torch
    n, T = 16, 8
    mk = lambda: wk.Engine(n, seed=SEED, RandomizeStart=1, Horizon=T, Minibatch=32, Epochs=2, MaxTimesteps=20)
    plain, drawn = mk(), mk()
    buf = torch.zeros(2 * 96 * 128 * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rec = R.synthetic_record()

    def draw(eng):
        eng.render([0, 5, 5], **WIN)
        eng.render_states(np.stack([rec, rec]), [1, 2], **WIN)
        eng.render_device(buf.data_ptr(), [3, 4], **WIN)

    for eng, do in ((plain, False), (drawn, True)):
        eng.profile_enable(True)
        for k in range(3):
            if do:
                draw(eng)
            eng.rollout()
            if do:
                draw(eng)
            if k == 1:
                eng.ppo_update(update_index=0)
                if do:
                    draw(eng)
    ta, tb = plain.get_trajectory(T), drawn.get_trajectory(T)
    for k in ta:
        assert ta[k].tobytes() == tb[k].tobytes(), k
    assert plain.get_weights().tobytes() == drawn.get_weights().tobytes()
    (ma, va, tta), (mb, vb, ttb) = plain.get_adam(), drawn.get_adam()
    assert ma.tobytes() == mb.tobytes() and va.tobytes() == vb.tobytes() and tta == ttb > 0
    assert plain.get_state().tobytes() == drawn.get_state().tobytes()
    sa, sb = plain.rollout_stats(), drawn.rollout_stats()
    for k in ("reward_sum", "episodes", "env_steps", "fault_or"):
        assert getattr(sa, k) == getattr(sb, k), k
    pa, pb = plain.profile(), drawn.profile()
    for k in ("physics_launches", "physics_env_steps", "returns_launches", "update_calls"):
        assert pa[k] == pb[k], k
    (ea, da), (eb, db) = plain.drain_episodes(), drawn.drain_episodes()
    assert len(ea) > 0 and ea.tobytes() == eb.tobytes() and da == db
    # and the frames show the trained walkers
    R.assert_shows(drawn.render([0], **WIN)[0], [R.WHITE, R.GRAY], "after training")
    plain.close()
    drawn.close()


def test_argument_errors_write_nothing(flat, wk):
    lib, h = flat.lib, flat.h
    good = wk.render_args(**WIN)
    ids = np.array([0, 1], np.int32)
    img = np.full((2, 96, 128, 4), 0xAB, np.uint8)
    st = np.zeros((2, wk.STATE_FLOATS), F)
    nan, inf = float("nan"), float("inf")

    def bad(**kw):
        return wk.render_args(**dict(WIN, **kw))

    def expect_error(call, text):
        assert call() == -1
        msg = lib.wk_last_error(h).decode()
        assert text in msg, (text, msg)
        assert (img == 0xAB).all()

    P = lambda a: a.ctypes.data
    render = lambda a, ids_=ids, n=2, out=P(img): lib.wk_render(h, C.byref(a) if a else None, P(ids_) if ids_ is not None else None, n, out)
    expect_error(lambda: render(None), "args is NULL")
    expect_error(lambda: render(good, None), "envs is NULL")
    expect_error(lambda: render(good, out=None), "image pointer is NULL")
    expect_error(lambda: lib.wk_render_states(h, C.byref(good), None, P(ids), 2, P(img)), "states is NULL")
    expect_error(lambda: lib.wk_render_device(h, C.byref(good), P(ids), 2, None), "image pointer is NULL")
    expect_error(lambda: render(good, n=0), "n_views 0")
    expect_error(lambda: render(good, n=-1), "n_views -1")
    expect_error(lambda: render(good, n=wk.RENDER_MAX_VIEWS + 1), "n_views 4097")
    expect_error(lambda: render(good, np.array([0, flat.n], np.int32)), "envs[1] = %d" % flat.n)
    expect_error(lambda: render(good, np.array([-1, 0], np.int32)), "envs[0] = -1")
    expect_error(lambda: lib.wk_render_states(h, C.byref(good), P(st), P(np.array([0, 99], np.int32)), 2, P(img)), "envs[1] = 99")
    for kw in (dict(width=0), dict(height=0), dict(width=wk.RENDER_MAX_DIM + 1), dict(height=-5)):
        expect_error(lambda: render(bad(**kw)), "frame")
    for v in (0.0, -1.0, nan, inf):
        expect_error(lambda: render(bad(scale=v)), "scale")
        expect_error(lambda: render(bad(line_px=v)), "line_px")
    for v in (nan, inf, -inf):
        expect_error(lambda: render(bad(ox=v)), "ox and oy")
        expect_error(lambda: render(bad(oy=v)), "ox and oy")
    for v in (-1, 2):
        expect_error(lambda: render(bad(follow=v)), "follow and joints")
        expect_error(lambda: render(bad(joints=v)), "follow and joints")
    # the context renders correctly afterwards
    check(flat, [0, 1], CARPET, WIN, [R.WHITE], what="after the errors")
    assert render(good) == 0 and (img[..., 3] == 255).all()
