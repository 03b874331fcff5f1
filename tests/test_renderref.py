"""CPU: tests/renderref.py -- the float32 restatement of the frame renderer's image that
tests/test_gpu_render.py holds the kernel to -- against cases derivable by hand."""
import numpy as np

import renderref as R

F = np.float32


def _lit(seg, w=9, h=6):
    return {(int(i), int(j)) for j, i in zip(*np.nonzero(R.cover(seg, w, h)))}


def test_horizontal_segment_is_half_open_at_the_far_end():
    # centres (i + 0.5, 2.5): t = 4 (i + 0.5 - 2) in [0, 16) for i = 2..5; cr = 0
    assert _lit((2, 2.5, 6, 2.5, R.WHITE, 1)) == {(2, 2), (3, 2), (4, 2), (5, 2)}


def test_reversed_segment_from_the_rule():
    # a = (6, 2.5), d = (-4, 0): t = -4 (i + 0.5 - 6) = 4 (5.5 - i) in [0, 16) for i = 2..5 (i = 1 gives
    # 18, i = 6 gives -2): the same four pixels, now half-open at x = 2
    assert _lit((6, 2.5, 2, 2.5, R.WHITE, 1)) == {(2, 2), (3, 2), (4, 2), (5, 2)}
    # ends on pixel centres: (2.5, 2.5) -> (5.5, 2.5) owns its first centre and not its last
    assert _lit((2.5, 2.5, 5.5, 2.5, R.WHITE, 1)) == {(2, 2), (3, 2), (4, 2)}
    assert _lit((5.5, 2.5, 2.5, 2.5, R.WHITE, 1)) == {(3, 2), (4, 2), (5, 2)}


def test_width_is_strict():
    # tau = 2 about y = 3: centres at distance 0.5 are inside, at 1.5 outside; tau = 1: |cr| = 0.5 |d|
    # is not < 0.5 |d|, so a segment on a pixel border lights nothing
    assert _lit((2, 3, 6, 3, R.WHITE, 2)) == {(i, j) for i in range(2, 6) for j in (2, 3)}
    assert _lit((2, 3, 6, 3, R.WHITE, 1)) == set()


def test_zero_length_and_nan_light_nothing():
    assert _lit((3, 3, 3, 3, R.WHITE, 5)) == set()
    nan, inf = float("nan"), float("inf")
    for seg in ((nan, 2.5, 6, 2.5), (2, nan, 6, 2.5), (2, 2.5, nan, 2.5), (2, 2.5, 6, nan),
                (inf, 2.5, 6, 2.5), (2, 2.5, inf, 2.5), (2, 2.5, 6, -inf), (1e30, 2.5, -1e30, 2.5)):
        assert _lit(seg + (R.WHITE, 1)) == set(), seg


def test_higher_index_wins_an_overlap():
    a, b = (1, 2.5, 7, 2.5, (10, 20, 30), 1), (4.5, 0, 4.5, 6, (40, 50, 60), 1)
    img = R.rasterize([a, b], 9, 6)
    assert tuple(img[2, 4]) == (40, 50, 60, 255) and tuple(img[2, 3]) == (10, 20, 30, 255)
    assert tuple(R.rasterize([b, a], 9, 6)[2, 4]) == (10, 20, 30, 255)
    assert tuple(img[0, 0]) == (0, 0, 0, 255) and (img[..., 3] == 255).all()


def test_joint_colours():
    assert R.joint_rgb(-1) == (0, 0, 255)
    assert R.joint_rgb(0) == (128, 0, 128)      # (int)(127.5 + 0.5)
    assert R.joint_rgb(1) == (255, 0, 0)
    assert R.joint_rgb(2) == (255, 0, 0) and R.joint_rgb(-7) == (0, 0, 255)
    assert R.joint_rgb(float("nan")) == (128, 0, 128)
    assert R.joint_rgb(float("inf")) == (255, 0, 0)
    assert R.joint_rgb(0.5) == (191, 0, 64)     # 0.75 * 255 = 191.25 -> 191; 0.25 * 255 = 63.75 -> 64


def test_follow_transform():
    a = R.args(width=96, height=96, scale=0.25, ox=0.0, follow=1)
    # the window is 384 units wide: a torso at x = 300 sits in the middle column
    assert R.view_origin(a, 300.0) == F(108)
    u, v = R.to_pixels(300.0, 400.0, a, R.view_origin(a, 300.0))
    assert (u, v) == (F(48), F(0))
    assert R.view_origin(R.args(ox=7.0), 300.0) == F(7)
    assert R.view_origin(R.args(width=550, scale=0.5, ox=-10.0, follow=1), 125.0) == F(125 - 550 - 10)


def test_painters_order_and_counts():
    rec = R.synthetic_record()
    segs = R.view_segments(rec, 0, R.args(marker_x=400.0))
    assert len(segs) == 16 + 1 + 4 + 29
    assert [s[4] for s in segs[:4]] == [(255, 0, 0)] * 4 and segs[16][4] == R.LIME
    assert segs[17][4] == R.WHITE and segs[21][4] == R.GRAY
    assert {float(s[5]) for s in segs[:17]} == {2.0} and {float(s[5]) for s in segs[17:]} == {1.0}
    assert len(R.view_segments(rec, 0, R.args(joints=0))) == 33
    rough = [R.FLAT_FLOOR] * 10
    sq = np.array([[1, 1], [0, 1], [0, 0], [1, 0]], F)
    segs = R.view_segments(rec, 4, R.args(), rough, [(sq, 1, 4), (sq, 0, 4)])
    assert len(segs) == 16 + 40 + 29 + 8
    assert [s[4] for s in segs[-8:]] == [R.WHITE] * 4 + [R.SANDYBROWN] * 4 and segs[56][4] == R.SANDYBROWN


def test_joint_square_corners():
    rec = R.synthetic_record()
    a = R.args(scale=1.0, ox=0.0, oy=0.0)
    segs = R.view_segments(rec, 0, a)
    pa, pb = R.body_vertices(rec, R.BODY)[1], R.body_vertices(rec, R.LLU)[4]
    cx, cy = (pa[0] + pb[0]) / F(2), (pa[1] + pb[1]) / F(2)
    corners = [(s[0], s[1]) for s in segs[:4]]
    assert corners == [(cx - F(1.5), cy - F(1.5)), (cx + F(1.5), cy - F(1.5)), (cx + F(1.5), cy + F(1.5)),
                       (cx - F(1.5), cy + F(1.5))]
    assert [(s[2], s[3]) for s in segs[:4]] == corners[1:] + corners[:1]


def test_a_synthetic_walker_shows():
    """the condition the GPU cases assert, on the default window and on a following one"""
    rec = R.synthetic_record(torques=(1.0, -1.0, 0.25, float("nan")))
    # (the default window shows the whole floor: one-pixel outlines light 0.4 % of it, so the cases
    # look closer; and they put the floor's top edge, y = 900, on a row of pixel centres: on a pixel
    # border, as at oy = 400 and scale 0.5, a one-pixel line lights nothing -- the width is strict)
    assert R.lit_fraction(R.render_view(rec, 1, R.args())) < 0.01
    img = R.render_view(rec, 1, R.args(width=128, height=96, oy=739.0, ox=0.0, follow=1, marker_x=340.0))
    assert img.shape == (96, 128, 4) and (img[..., 3] == 255).all()
    R.assert_shows(img, [R.WHITE, R.CYAN, R.LIME, (255, 0, 0), (0, 0, 255), (128, 0, 128)], "half scale")
    close = R.args(width=128, height=96, scale=1.0, oy=819.5, ox=0.0, follow=1)
    img = R.render_view(rec, 6, close)
    R.assert_shows(img, [R.WHITE, R.SLATEGRAY, (255, 0, 0)], "follow")
    assert R.lit_fraction(R.rasterize([], 8, 8)) == 0.0
