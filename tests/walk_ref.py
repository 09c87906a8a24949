"""A plain restatement, in Python floats (IEEE f64, one rounding per operation, no contraction), of what the reference's
HitableList::hit, Sphere::hit, MovingSphere::hit, the three rectangles, Cube::hit and ConstantMedium::hit do to ONE ray -- for the
list-rooted scenes of tests/walk_cases.py.  It takes its random numbers from oracle.rng_f64 and its logarithm from the oracle's det_ln;
everything else is written out here, operation by operation in the order of oracle/rt_oracle.cpp, so that it must agree with
oracle.Scene.walk bit for bit (tests/test_walk_cases.py).  A difference is a finding about one of the two.

Scenes are the descriptions of walk_cases.py: ("sphere", c, r), ("msphere", c0, c1, t0, t1, r), ("rect", axis, a0, b0, a1, b1, k),
("cube", mn, mx), ("list", [..]), ("medium", density, boundary).  Transforms, meshes and BVH nodes are not restated (restatable()).

classify() also says what a row exercises of the device's traverse2_media: the media the ray crosses (both boundary queries answer),
where the closest surface S sits in the list, and for every third-or-later crossed medium M which of the three sub-cases applies --
"s_before" (S is listed before M), "limit_walk" (S after M, S.t below M's exit: the order-restricted walk runs), "beyond_exit" (S after M,
at or beyond the exit: nothing clips).  The restricted walk, and for the first two crossed media the widened candidate range of the
tracking walk (track_bound), change the answer only where a surface listed BEFORE the medium lies behind S and in front of the
medium's exit: "limit_clips" / "track_clips" mark those rows."""
import math

INF = math.inf
NAN = math.nan
CUBE_SIDES = ((2, 0, 1, 0), (2, 0, 1, 1), (1, 0, 2, 0), (1, 0, 2, 1), (0, 1, 2, 0), (0, 1, 2, 1))  # (axis, a, b, min/max) cube.rs:16-61


def fdiv(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def restatable(d):
    if d[0] in ("sphere", "msphere", "rect", "cube"):
        return True
    if d[0] == "list":
        return all(restatable(x) for x in d[1])
    if d[0] == "medium":
        return restatable(d[2])
    return False


class Stream:
    """the row's random stream: gen_f64 number by number, counted"""

    def __init__(self, key):
        self.key = [int(k) for k in key]
        self.draws = 0
        self.buf = None

    def gen_f64(self):
        import oracle
        if self.buf is None or self.draws >= len(self.buf):
            self.buf = oracle.rng_f64(self.key[0], self.key[1], self.key[2], 16 if self.buf is None else 4 * len(self.buf))
        x = float(self.buf[self.draws])
        self.draws += 1
        return x


def _sphere(o, d, c, radius, t_min, t_max):
    ocx, ocy, ocz = o[0] - c[0], o[1] - c[1], o[2] - c[2]
    a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    half_b = ocx * d[0] + ocy * d[1] + ocz * d[2]
    cc = (ocx * ocx + ocy * ocy + ocz * ocz) - radius * radius
    disc = half_b * half_b - a * cc
    if disc < 0.0:
        return None
    sq = math.sqrt(disc) if disc == disc else NAN
    root = fdiv(-half_b - sq, a)
    if not (root >= t_min and root <= t_max):
        root = fdiv(-half_b + sq, a)
    if not (root >= t_min and root <= t_max):
        return None
    return root


def _rect(o, d, axis, a0, b0, a1, b1, k, t_min, t_max):
    t = fdiv(k - o[axis], d[axis])
    if t < t_min or t > t_max:
        return None
    p = (o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t)
    if axis == 2:
        a, b = p[0], p[1]
    elif axis == 1:
        a, b = p[0], p[2]
    else:
        a, b = p[1], p[2]
    if a < a0 or a > a1 or b < b0 or b > b1:
        return None
    return t


def hit(desc, o, d, time, t_min, t_max, stream):
    """-> t of desc's hit in [t_min, t_max], or None"""
    kind = desc[0]
    if kind == "sphere":
        return _sphere(o, d, desc[1], desc[2], t_min, t_max)
    if kind == "msphere":
        _, c0, c1, t0, t1, radius = desc
        s = fdiv(time - t0, t1 - t0)
        c = (c0[0] + (c1[0] - c0[0]) * s, c0[1] + (c1[1] - c0[1]) * s, c0[2] + (c1[2] - c0[2]) * s)
        return _sphere(o, d, c, radius, t_min, t_max)
    if kind == "rect":
        return _rect(o, d, desc[1], desc[2], desc[3], desc[4], desc[5], desc[6], t_min, t_max)
    if kind == "cube":
        mn, mx = desc[1], desc[2]
        closest, best = t_max, None
        for axis, ia, ib, side in CUBE_SIDES:
            t = _rect(o, d, axis, mn[ia], mn[ib], mx[ia], mx[ib], (mx if side else mn)[axis], t_min, closest)
            if t is not None:
                closest = best = t
        return best
    if kind == "list":
        closest, best = t_max, None
        for x in desc[1]:
            t = hit(x, o, d, time, t_min, closest, stream)
            if t is not None:
                closest = best = t
        return best
    if kind == "medium":
        import oracle
        _, density, boundary = desc
        t1 = hit(boundary, o, d, time, -INF, INF, stream)
        if t1 is None:
            return None
        t2 = hit(boundary, o, d, time, t1 + 0.0001, INF, stream)
        if t2 is None:
            return None
        t1 = fmax(t1, t_min)
        t2 = fmin(t2, t_max)
        if t1 >= t2:
            return None
        t1 = fmax(t1, 0.0)
        ray_length = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        inside = (t2 - t1) * ray_length
        hit_distance = (-1.0 / density) * oracle.det_ln(stream.gen_f64())
        if hit_distance > inside:
            return None
        return t1 + fdiv(hit_distance, ray_length)
    raise ValueError("walk_ref does not restate %r" % (kind,))


def walk(items, ray7, key, t_min):
    """HitableList(items).hit(ray, t_min, +inf) with a fresh stream of `key` -> (hit, t, winning list index or -1, draws)"""
    o, d, time = tuple(float(x) for x in ray7[0:3]), tuple(float(x) for x in ray7[3:6]), float(ray7[6])
    stream = Stream(key)
    closest, win = INF, -1
    for k, x in enumerate(items):
        t = hit(x, o, d, time, t_min, closest, stream)
        if t is not None:
            closest, win = t, k
    return win >= 0, (closest if win >= 0 else 0.0), win, stream.draws


def classify(items, ray7, t_min):
    """-> dict(crossed = list indices of the media whose two boundary queries answer, s_index = list index of the closest surface (-1:
    none), s_t, cases = the set of sub-cases of the third-or-later crossed media)"""
    o, d, time = tuple(float(x) for x in ray7[0:3]), tuple(float(x) for x in ray7[3:6]), float(ray7[6])
    s_t, s_index = INF, -1
    for k, x in enumerate(items):
        if x[0] == "medium":
            continue
        t = hit(x, o, d, time, t_min, s_t, None)
        if t is not None:
            s_t, s_index = t, k
    crossed, cases = [], set()
    for k, x in enumerate(items):
        if x[0] != "medium":
            continue
        t1 = hit(x[2], o, d, time, -INF, INF, None)
        t2 = hit(x[2], o, d, time, t1 + 0.0001, INF, None) if t1 is not None else None
        if t2 is None:
            continue
        crossed.append(k)
        if s_index < 0:
            continue
        before_t = INF                      # the closest surface among those listed before the medium
        for y in items[:k]:
            if y[0] != "medium":
                t = hit(y, o, d, time, t_min, before_t, None)
                before_t = before_t if t is None else t
        clips = s_index > k and s_t < before_t < t2         # ... lies behind S and still inside the medium: only a walk that looks past S finds it
        if len(crossed) >= 3:
            cases.add("s_before" if s_index < k else "limit_walk" if s_t < t2 else "beyond_exit")
            if clips:
                cases.add("limit_clips")
        elif clips:
            cases.add("track_clips")
    return dict(crossed=crossed, s_index=s_index, s_t=s_t, cases=cases)
