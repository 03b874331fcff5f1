"""The frame renderer's image (include/wk_api.h, "Frames") restated in float32 numpy: the
transform, the coverage rule of one segment, the painter's order, the colours.  Every product,
sum and comparison is the one the rule names, in fp32 and unfused, so the kernel's frames must equal
these in every byte (tests/test_gpu_render.py); tests/test_renderref.py checks this file against
cases derivable by hand."""
import numpy as np

F = np.float32
NSTATE, BSTRIDE, ST_TORQUE, ST_POS = 112, 20, 100, 104
LLL, LLU, BODY, RLL, RLU = range(5)
NVERT = (6, 6, 5, 6, 6)

BLACK, WHITE, LIME, GRAY = (0, 0, 0), (255, 255, 255), (0, 255, 0), (128, 128, 128)
CYAN, SANDYBROWN, SLATEGRAY = (0, 255, 255), (244, 164, 96), (112, 128, 144)
# Materials/<Name>.cs GetColor(), by wk_material id: Carpet Ice Rubber Metal Wood Paper Titanium SuperRubber
MATERIAL_RGB = (GRAY, CYAN, GRAY, WHITE, SANDYBROWN, GRAY, SLATEGRAY, GRAY)
# Walker._joints (Walker.cs:182-187): (body, vertex) of point A and of point B
JOINTS = (((BODY, 1), (LLU, 4)), ((BODY, 1), (RLU, 4)), ((LLU, 2), (LLL, 3)), ((RLU, 2), (RLL, 3)))
FLAT_FLOOR = np.array([[-50, 1050], [-50, 900], [1050, 900], [1050, 1050]], F)

DEFAULTS = dict(width=550, height=325, scale=0.5, ox=-50.0, oy=400.0, follow=0, line_px=1.0,
                marker_x=float("nan"), joints=1)


def args(**kw):
    a = dict(DEFAULTS)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return a


def joint_rgb(torque):
    """value = (1f + clamp(torque, -1, 1)) / 2f; R = (int)(value 255f + 0.5f), G = 0,
    B = (int)((1f - value) 255f + 0.5f); a NaN torque counts as 0"""
    t = F(torque)
    if np.isnan(t):
        t = F(0)
    t = F(-1) if t < F(-1) else (F(1) if t > F(1) else t)
    value = F(F(1) + t) / F(2)
    return (int(F(F(value * F(255)) + F(0.5))), 0, int(F(F(F(F(1) - value) * F(255)) + F(0.5))))


def view_origin(a, posx):
    """ox_view: ox, or with follow (posx - 0.5f * ((float)width / scale)) + ox"""
    if not a["follow"]:
        return F(a["ox"])
    return F(F(F(posx) - F(F(0.5) * F(F(a["width"]) / F(a["scale"])))) + F(a["ox"]))


def to_pixels(x, y, a, oxv):
    s = F(a["scale"])
    return F(F(F(x) - oxv) * s), F(F(F(y) - F(a["oy"])) * s)


def body_vertices(rec, b):
    return np.asarray(rec, F)[b * BSTRIDE:b * BSTRIDE + 2 * NVERT[b]].reshape(-1, 2)


def view_segments(rec, material, a, floor=(FLAT_FLOOR,), props=()):
    """The segments of one view in painter's order, in pixel coordinates: a list of
    (ax, ay, bx, by, rgb, tau).  floor: the floor's polygons ([4, 2] arrays: the flat floor, or the
    10 rough segments in order); props: (vertices [nv, 2], is_static, material id) in scene order."""
    rec = np.asarray(rec, F)
    oxv = view_origin(a, rec[ST_POS])
    tau, tau2 = F(a["line_px"]), F(F(2) * F(a["line_px"]))
    out = []

    def seg(p, q, rgb, t):
        au, av = to_pixels(p[0], p[1], a, oxv)
        bu, bv = to_pixels(q[0], q[1], a, oxv)
        out.append((au, av, bu, bv, rgb, t))

    def polygon(v, rgb, t):
        for k in range(len(v)):
            seg(v[k], v[(k + 1) % len(v)], rgb, t)

    if a["joints"]:
        for k, ((ba, va), (bb, vb)) in enumerate(JOINTS):
            pa, pb = body_vertices(rec, ba)[va], body_vertices(rec, bb)[vb]
            # Renderer.DrawSquare(centre, 3): squareOrigin = centre - 3 / 2
            sx = F(F(F(pa[0] + pb[0]) / F(2)) - F(1.5))
            sy = F(F(F(pa[1] + pb[1]) / F(2)) - F(1.5))
            sq = [(sx, sy), (F(sx + F(3)), sy), (F(sx + F(3)), F(sy + F(3))), (sx, F(sy + F(3)))]
            polygon(sq, joint_rgb(rec[ST_TORQUE + k]), tau2)
    if not np.isnan(F(a["marker_x"])):
        seg((F(a["marker_x"]), F(500)), (F(a["marker_x"]), F(900)), LIME, tau2)
    for v in floor:
        polygon(np.asarray(v, F), WHITE, tau)
    for b in (LLL, LLU, BODY, RLL, RLU):
        polygon(body_vertices(rec, b), MATERIAL_RGB[material], tau)
    for v, is_static, mat in props:
        polygon(np.asarray(v, F), WHITE if is_static else MATERIAL_RGB[mat], tau)
    return out


def cover(seg, width, height):
    """bool [height, width]: the pixels segment (ax, ay, bx, by, ., tau) covers.  d = b - a, L2 = d.d,
    c = (i + 0.5f, j + 0.5f), e = c - a, t = e.d, cr = e x d; covered exactly when L2 > 0, t >= 0,
    t < L2 and cr cr < (0.25f tau tau) L2"""
    ax, ay, bx, by, _, tau = seg
    ax, ay, bx, by, tau = F(ax), F(ay), F(bx), F(by), F(tau)
    with np.errstate(all="ignore"):
        dx, dy = F(bx - ax), F(by - ay)
        l2 = F(F(dx * dx) + F(dy * dy))
        thr = F(F(F(F(0.25) * tau) * tau) * l2)
        cx = (np.arange(width, dtype=F) + F(0.5))[None, :]
        cy = (np.arange(height, dtype=F) + F(0.5))[:, None]
        ex, ey = cx - ax, cy - ay
        t = ex * dx + ey * dy
        cr = ex * dy - ey * dx
        assert t.dtype == F and cr.dtype == F
        return (l2 > F(0)) & (t >= F(0)) & (t < l2) & (cr * cr < thr)


def rasterize(segs, width, height):
    """uint8 [height, width, 4]: black, A = 255, then every segment in order (the highest covering
    index gives the colour)"""
    img = np.zeros((height, width, 4), np.uint8)
    img[..., 3] = 255
    for s in segs:
        img[cover(s, width, height), :3] = s[4]
    return img


def render_view(rec, material, a, floor=(FLAT_FLOOR,), props=()):
    return rasterize(view_segments(rec, material, a, floor, props), a["width"], a["height"])


def lit_fraction(img):
    return float((img[..., :3] != 0).any(axis=-1).mean())


def has_colour(img, rgb):
    return bool((img[..., :3] == np.array(rgb, np.uint8)).all(axis=-1).any())


def has_joint_colour(img):
    """a joint square's (R, 0, B): no other colour of the table has G = 0"""
    rgb = img[..., :3].astype(np.int32)
    return bool(((rgb[..., 1] == 0) & (rgb[..., 0] + rgb[..., 2] > 0)).any())


def assert_shows(img, colours, what=""):
    """the condition that keeps two black frames from passing: at least 1 % of the pixels lit, and
    every colour the case is about present"""
    assert lit_fraction(img) >= 0.01, (what, lit_fraction(img))
    for rgb in colours:
        assert has_colour(img, rgb), (what, rgb)


def pole(cx, cy, half_len, half_w, angle):
    """six vertices of a thin hexagonal pole about (cx, cy): a stand-in for Pole.FromSize's shape"""
    loc = np.array([[-half_w, -half_len], [0, -half_len - half_w], [half_w, -half_len],
                    [half_w, half_len], [0, half_len + half_w], [-half_w, half_len]], np.float64)
    c, s = np.cos(angle), np.sin(angle)
    return (loc @ np.array([[c, s], [-s, c]]) + [cx, cy]).astype(F)


def synthetic_record(x=300.0, torques=(1.0, -1.0, 0.25, 0.0)):
    """A hand-built walker record standing on the flat floor at torso x: four poles and a pentagon
    where a walker's would be (not a physical state: wk_render_states only draws)."""
    rec = np.zeros(NSTATE, F)
    parts = {LLU: pole(x - 6, 835, 18, 4, 0.15), LLL: pole(x - 9, 877, 18, 4, -0.05),
             RLU: pole(x + 6, 835, 18, 4, -0.2), RLL: pole(x + 10, 877, 18, 4, 0.1)}
    for b, v in parts.items():
        rec[b * BSTRIDE:b * BSTRIDE + 12] = v.reshape(-1)
    torso = np.array([[x - 20, 815], [x, 822], [x + 20, 815], [x + 14, 770], [x - 14, 770]], F)
    rec[BODY * BSTRIDE:BODY * BSTRIDE + 10] = torso.reshape(-1)
    rec[ST_TORQUE:ST_TORQUE + 4] = torques
    rec[ST_POS], rec[ST_POS + 1] = x, 800
    return rec
