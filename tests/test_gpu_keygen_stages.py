"""GPU: the per-point map of key generation (lurk_beta_amd/csrc/keygen_point.cuh) stage by stage, one case per lane, against
hashlib, Python integers and the stage functions of oracle/keygen_ref.py.  Exact integers everywhere: there is no tolerance.

tests/test_gpu_keygen.py feeds messages through the whole map, which pins the generic path; the branches below are steered by
BLAKE2b outputs nobody can choose, so they are driven here at the stage level: the reduction's boundaries (halves in [p, 2p),
[2p, 3p), [3p, 2^256)), every Tonelli-Shanks loop depth (and waves whose lanes differ in depth), the SWU exceptional case u = 0,
the doubling and the cancellation in the affine addition, the isogeny's kernel, and b2b_hash at exactly one and exactly two blocks.

tests/gpu_keygen/keygen_probe.hip is built once per module with the Makefile's CXXFLAGS and runs once as a child process:
inputs go in through a file, outputs come back through one.  It runs every set on the device with 128 and with 64 threads per
block and on the host (the code of lurk_hip_ck_from_label_host) and exits non-zero unless the three are identical bytes.  Its
host pass runs first, compiled with LURK_FE_CHECK: a stage that hands fe_mul / fe_add / fe_sub an operand >= p aborts the probe
before it touches the device, and every test here then fails in the fixture.  Every test asserts that it compared as many cases
as it sent."""
import functools
import hashlib
import os
import random
import re
import shutil
import struct
import subprocess

import pytest

from oracle import keygen_ref as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "gpu_keygen", "keygen_probe.hip")
CURVES = ["pallas", "vesta"]
OPS = {name: i for i, name in enumerate(["b2b_hash", "from_be64", "is_square", "sqrt", "hash_to_field", "map_to_curve", "iso_add",
                                         "iso_map", "point"])}
IN_BYTES = dict(b2b_hash=260, from_be64=64, is_square=32, sqrt=32, hash_to_field=64, map_to_curve=64, iso_add=128, iso_map=64, point=64)
OUT_BYTES = dict(b2b_hash=64, from_be64=32, is_square=4, sqrt=32, hash_to_field=64, map_to_curve=128, iso_add=68, iso_map=64, point=64)
SUITE = K.CK_DEFAULTS["suite"]


def tag_configs(cn):
    """(name, domain prefix, msg_len): the default tag; the longest admissible tag (62 bytes) with 62-byte messages, so that the
    first hash is exactly 256 bytes and the other two exactly 128; a one-byte message under a one-character prefix"""
    name = K.CK_DEFAULTS["curve_name_" + cn]
    longest = "L" * (62 - 1 - len(name) - len(SUITE))
    assert len(f"{longest}-{name}{SUITE}") == 62 and 131 + 62 + 63 == 256 and 65 + 63 == 128
    return [("default", K.CK_DEFAULTS["domain_prefix"], 32), ("longest", longest, 62), ("short", "x", 1)]


# ---- the fields ---------------------------------------------------------------------------------------------------------------
def fe(v):
    return int(v).to_bytes(32, "little")


def ints(rec, k):
    return tuple(int.from_bytes(rec[32 * i:32 * (i + 1)], "little") for i in range(k))


def modulus(cn):
    return K.CURVE[cn]["p"]


@functools.lru_cache(None)
def two_adic(cn):
    """(z, T, w): the smallest non-residue, the odd part of p - 1 = 2^32 T, and w = z^T of order 2^32"""
    p = modulus(cn)
    z = 2
    while K.is_square(z, p):
        z += 1
    assert z == 5 and (p - 1) % (1 << 32) == 0 and ((p - 1) >> 32) % 2 == 1
    T = (p - 1) >> 32
    return z, T, pow(z, T, p)


def depth_family(cn, rng=None):
    """w^(2^j), j = 0..32: the order of (w^(2^j))^T is 2^(32-j), so j = 1..32 are squares, one for every loop depth of kg_sqrt
    (j = 32 is a = 1: t == 1 on entry) and j = 0 is a non-residue.  With rng: each times a seeded element of odd order."""
    p = modulus(cn)
    _, _, w = two_adic(cn)
    fam = [pow(w, 1 << j, p) for j in range(33)]
    if rng is not None:
        fam = [x * pow(rng.randrange(2, p), 1 << 32, p) % p for x in fam]
    return fam


def g_iso(cn, x):
    c = K.CURVE[cn]
    return (x * x * x + c["a"] * x + c["b"]) % c["p"]


def gx1_is_square(cn, u):
    """which branch of simplified SWU u takes (the oracle's formulas up to the Legendre symbol)"""
    c = K.CURVE[cn]
    p = c["p"]
    z_u2 = c["z"] * u * u % p
    ta = (z_u2 * z_u2 + z_u2) % p
    x1 = c["b"] * (ta + 1) * pow(c["a"] * (c["z"] if ta == 0 else -ta), p - 2, p) % p
    return K.is_square(g_iso(cn, x1), p)


def iso_kernel_x(cn):
    c = K.CURVE[cn]
    return -c["iso"][4] * pow(2, -1, c["p"]) % c["p"]


# ---- the case sets ------------------------------------------------------------------------------------------------------------
B2B_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 255, 256]


@functools.lru_cache(None)
def b2b_cases():
    rng = random.Random(0xB2B)
    msgs = []
    for n in B2B_LENGTHS:
        msgs += [bytes(n), b"\xff" * n, rng.randbytes(n)]
    msgs += [rng.randbytes(rng.randrange(0, 257)) for _ in range(256)]
    return msgs


@functools.lru_cache(None)
def from_be64_cases(cn):
    p = modulus(cn)
    rng = random.Random(0xBE64 + len(cn))
    halves = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p - 1, 3 * p, 3 * p + 1, (1 << 256) - 1]
    assert all(0 <= h < 1 << 256 for h in halves)
    vals = []
    for h in halves:
        vals += [h, h << 256, h << 256 | h]  # low half, high half, both
    return [v.to_bytes(64, "big") for v in vals] + [rng.randbytes(64) for _ in range(1024)]


@functools.lru_cache(None)
def is_square_cases(cn):
    p = modulus(cn)
    z = two_adic(cn)[0]
    rng = random.Random(0x15C + len(cn))
    vals = [0, 1, p - 1, 4, z, z * z] + depth_family(cn) + depth_family(cn, rng)
    vals += [pow(rng.randrange(1, p), 2, p) for _ in range(1024)]
    vals += [z * pow(rng.randrange(1, p), 2, p) % p for _ in range(1024)]
    return vals


@functools.lru_cache(None)
def sqrt_cases(cn):
    p = modulus(cn)
    z = two_adic(cn)[0]
    rng = random.Random(0x5C27 + len(cn))
    vals = [0, 1, p - 1, 4, z * z] + depth_family(cn)[1:] + depth_family(cn, rng)[1:]
    return vals + [pow(rng.randrange(1, p), 2, p) for _ in range(1024)]


@functools.lru_cache(None)
def sqrt_layouts(cn):
    """mixed: every wave of 64 lanes holds the 32 depths twice (the pure powers, then the same times odd-order elements): no two
    neighbouring lanes run the same number of rounds and the wave runs the longest.  uniform: wave d holds 64 different squares of
    depth d, so every lane of a wave runs the same rounds; its lanes 0 and 1 are the mixed layout's two elements of that depth, and
    the per-element results must be the same bytes in both layouts."""
    p = modulus(cn)
    rng = random.Random(0x1A70 + len(cn))
    pure, odd = depth_family(cn)[1:], depth_family(cn, rng)[1:]
    mixed = (pure + odd) * 4
    uniform = []
    for d in range(32):
        uniform += [pure[d], odd[d]] + [pure[d] * pow(rng.randrange(2, p), 1 << 32, p) % p for _ in range(62)]
    assert len(mixed) == 256 and len(uniform) == 2048
    return mixed, uniform


@functools.lru_cache(None)
def map_to_curve_cases(cn):
    p = modulus(cn)
    rng = random.Random(0x5111 + len(cn))
    u = rng.randrange(2, p)
    sq = [x for x in (rng.randrange(1, p) for _ in range(64)) if gx1_is_square(cn, x)][:2]
    ns = [x for x in (rng.randrange(1, p) for _ in range(64)) if not gx1_is_square(cn, x)][:2]
    assert len(sq) == 2 and len(ns) == 2
    pairs = [(0, 0), (0, u), (u, 0), (u, u), (u, p - u), (1, p - 1), (sq[0], ns[0]), (ns[1], sq[1]), (sq[0], sq[1]), (ns[0], ns[1])]
    seeded = [(rng.randrange(p), rng.randrange(p)) for _ in range(1024)]
    kinds = {gx1_is_square(cn, a) for a, _ in seeded[:64]}
    assert kinds == {True, False}  # both branches among the seeded pairs too
    return pairs + seeded


@functools.lru_cache(None)
def iso_add_cases(cn):
    """[(q0, q1, kind)], points from the oracle's simplified SWU.  The first 64 lanes interleave the three kinds within one wave."""
    p = modulus(cn)
    rng = random.Random(0xADD + len(cn))
    pt = lambda: K.map_to_curve_simple_swu(cn, rng.randrange(p))
    neg = lambda q: (q[0], (-q[1]) % p)

    def case(kind):
        q = pt()
        return (q, pt(), kind) if kind == "generic" else (q, q, kind) if kind == "double" else (q, neg(q), kind)

    kinds = ["generic", "double", "negate"]
    cases = [case(kinds[i % 3]) for i in range(64)]
    for kind in kinds:
        cases += [case(kind) for _ in range(8)]
    return cases + [case("generic") for _ in range(512)]


@functools.lru_cache(None)
def iso_map_cases(cn):
    """[((x, y), on the isogenous curve?)]: the sums of the iso_add cases, the kernel abscissa x0 with three ordinates, and its
    neighbours.  No point of the isogenous curve has x = x0 (g(x0) is a non-residue); a neighbour gets the ordinate that puts it on
    the curve where one exists (g(x0 +- 1) is a non-residue on Pallas' isogenous curve and a square on Vesta's), and the nearest
    abscissa on either side that does carry a point is added, so both curves have on-curve inputs next to the kernel."""
    p = modulus(cn)
    cases = []
    for q0, q1, _ in iso_add_cases(cn):
        s = K.iso_add(cn, q0, q1)
        if s is not None:
            cases.append((s, True))
    x0 = iso_kernel_x(cn)
    assert not K.is_square(g_iso(cn, x0), p)
    cases += [((x0, y), False) for y in (0, 1, p - 1)]
    for step in (1, -1):
        x = (x0 + step) % p
        y = K.sqrt_mod(g_iso(cn, x), p)
        cases.append(((x, 1), False) if y is None else ((x, y), True))
        while K.sqrt_mod(g_iso(cn, x), p) is None:
            x = (x + step) % p
        cases.append(((x, K.sqrt_mod(g_iso(cn, x), p)), True))
    return cases


@functools.lru_cache(None)
def messages(cn, cfg, msg_len):
    rng = random.Random(f"{cn}/{cfg}")
    return [bytes(msg_len), b"\xff" * msg_len] + [rng.randbytes(msg_len) for _ in range(62)]


@functools.lru_cache(None)
def all_sets():
    """[(curve name, set name, op, prefix, msg_len, [input record])], every record IN_BYTES[op] long"""
    sets = []
    for cn in CURVES:
        dflt = ("default", K.CK_DEFAULTS["domain_prefix"], 32)
        add = lambda name, op, recs, cfg=dflt: sets.append((cn, name, op, cfg[1], cfg[2], recs))
        add("b2b_hash", "b2b_hash", [struct.pack("<I", len(m)) + m.ljust(256, b"\0") for m in b2b_cases()])
        add("from_be64", "from_be64", from_be64_cases(cn))
        add("is_square", "is_square", [fe(v) for v in is_square_cases(cn)])
        add("sqrt", "sqrt", [fe(v) for v in sqrt_cases(cn)])
        mixed, uniform = sqrt_layouts(cn)
        add("sqrt mixed depths", "sqrt", [fe(v) for v in mixed])
        add("sqrt uniform depths", "sqrt", [fe(v) for v in uniform])
        add("map_to_curve", "map_to_curve", [fe(a) + fe(b) for a, b in map_to_curve_cases(cn)])
        add("iso_add", "iso_add", [fe(q0[0]) + fe(q0[1]) + fe(q1[0]) + fe(q1[1]) for q0, q1, _ in iso_add_cases(cn)])
        add("iso_map", "iso_map", [fe(x) + fe(y) for (x, y), _ in iso_map_cases(cn)])
        for cfg in tag_configs(cn):
            recs = [m.ljust(64, b"\0") for m in messages(cn, cfg[0], cfg[2])]
            add("hash_to_field " + cfg[0], "hash_to_field", recs, cfg)
            add("point " + cfg[0], "point", recs, cfg)
    for cn, name, op, _, _, recs in sets:
        assert recs and all(len(r) == IN_BYTES[op] for r in recs), (cn, name)
        assert len(recs) <= 2200  # the largest set is about 2 000 lanes
    return sets


# ---- the probe ----------------------------------------------------------------------------------------------------------------
def hipcc():
    path = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(path), "hipcc not found: the probe cannot be built"
    return path


def makefile_cxxflags():
    mk = open(os.path.join(ROOT, "lurk_beta_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def write_input(path, sets):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(sets)))
        for cn, _, op, prefix, msg_len, recs in sets:
            name = K.CK_DEFAULTS["curve_name_" + cn]
            f.write(struct.pack("<IIII64s16s32s", CURVES.index(cn), OPS[op], len(recs), msg_len, prefix.encode(), name.encode(), SUITE.encode()))
            f.write(b"".join(recs))


class ProbeRun:
    def __init__(self, returncode, text, out):
        self.returncode, self.text, self.out = returncode, text, out

    def records(self, cn, name):
        recs, inputs = self.out[cn, name]
        assert len(recs) == len(inputs)  # nothing dropped on the GPU side
        return recs, inputs


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("keygen_probe"))
    exe = os.path.join(tmp, "keygen_probe")
    subprocess.run([hipcc(), *makefile_cxxflags(), "-o", exe, PROBE], cwd=tmp, check=True, timeout=600)
    sets = all_sets()
    inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    write_input(inp, sets)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=240)
    # 5: the three runs of a set disagree - the output (the 128-thread run) is complete, the stage tests still say which case is
    # wrong, and test_block_sizes_and_the_host_agree fails
    assert r.returncode in (0, 5), f"probe exit {r.returncode}: {r.stdout}{r.stderr}"
    data = open(outp, "rb").read()
    assert len(data) == sum(len(recs) * OUT_BYTES[op] for _, _, op, _, _, recs in sets), "probe output has the wrong size"
    out, off = {}, 0
    for cn, name, op, _, _, recs in sets:
        ob = OUT_BYTES[op]
        out[cn, name] = ([data[off + i * ob:off + (i + 1) * ob] for i in range(len(recs))], recs)
        off += len(recs) * ob
    return ProbeRun(r.returncode, r.stdout + r.stderr, out)


def test_block_sizes_and_the_host_agree(probe):
    """128 threads per block (the kernel's launch bound), 64 threads per block and the host loop: identical bytes for every set"""
    assert probe.returncode == 0, probe.text
    assert f"sets {len(all_sets())}, disagreements 0" in probe.text


# ---- stage by stage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", CURVES)
def test_b2b_hash_one_and_two_blocks(probe, cn):
    got, _ = probe.records(cn, "b2b_hash")
    msgs = b2b_cases()
    assert len(msgs) == 3 * len(B2B_LENGTHS) + 256 == len(got)
    assert {len(m) for m in msgs} >= set(B2B_LENGTHS)
    bad = [len(m) for m, g in zip(msgs, got) if g != hashlib.blake2b(m, digest_size=64).digest()]
    assert not bad, f"wrong digests at lengths {bad[:8]}"


@pytest.mark.parametrize("cn", CURVES)
def test_from_be64_at_the_reduction_boundaries(probe, cn):
    got, sent = probe.records(cn, "from_be64")
    p = modulus(cn)
    assert len(sent) == 36 + 1024
    bad = [(b.hex(), hex(ints(g, 1)[0])) for b, g in zip(sent, got) if ints(g, 1)[0] != int.from_bytes(b, "big") % p]
    assert not bad, bad[:4]


@pytest.mark.parametrize("cn", CURVES)
def test_is_square(probe, cn):
    got, _ = probe.records(cn, "is_square")
    p = modulus(cn)
    vals = is_square_cases(cn)
    assert len(vals) == 6 + 33 + 33 + 2048 == len(got)
    want = [K.is_square(v, p) for v in vals]
    assert want[:6] == [True, True, True, True, False, True]          # 0, 1, -1, 4, the smallest non-residue, its square
    assert want[6:39] == [False] + [True] * 32 == want[39:72]        # w^(2^j): j = 0 is the non-residue w itself
    assert want[72:] == [True] * 1024 + [False] * 1024
    bad = [hex(v) for v, g, w in zip(vals, got, want) if struct.unpack("<I", g)[0] != int(w)]
    assert not bad, bad[:4]


def check_roots(cn, vals, got):
    """a root r is right iff r^2 = a and r is the oracle's root or its negative (sgn0 fixes the sign later: map_to_curve checks it)"""
    p = modulus(cn)
    assert len(vals) == len(got)
    bad = []
    for a, g in zip(vals, got):
        r, want = ints(g, 1)[0], K.sqrt_mod(a, p)
        assert want is not None  # the oracle defines every input: all are squares
        if not (r < p and r * r % p == a and r in (want, (p - want) % p)):
            bad.append((hex(a), hex(r), hex(want)))
    assert not bad, bad[:4]
    return len(got)


@pytest.mark.parametrize("cn", CURVES)
def test_sqrt_at_every_loop_depth(probe, cn):
    got, _ = probe.records(cn, "sqrt")
    p = modulus(cn)
    vals = sqrt_cases(cn)
    assert check_roots(cn, vals, got) == 5 + 32 + 32 + 1024
    # the family covers every depth: the order of a^T is 2^(32-j) for j = 1..32
    T = two_adic(cn)[1]
    for fam in (vals[5:37], vals[37:69]):
        orders = []
        for a in fam:
            t, k = pow(a, T, p), 0
            while t != 1:
                t, k = t * t % p, k + 1
            orders.append(k)
        assert orders == list(range(31, -1, -1))
    assert vals[36] == 1 and ints(got[0], 1)[0] == 0  # a = 1: t == 1 on entry; a = 0


@pytest.mark.parametrize("cn", CURVES)
def test_sqrt_does_not_depend_on_the_lanes_beside_it(probe, cn):
    mixed, uniform = sqrt_layouts(cn)
    got_m, _ = probe.records(cn, "sqrt mixed depths")
    got_u, _ = probe.records(cn, "sqrt uniform depths")
    assert check_roots(cn, mixed, got_m) == 256 and check_roots(cn, uniform, got_u) == 2048
    compared = 0
    for d in range(32):  # the same element in a wave of 64 different rounds and in a wave where all lanes run depth d
        for w in range(4):
            assert got_m[64 * w + d] == got_u[64 * d] and got_m[64 * w + 32 + d] == got_u[64 * d + 1], d
            compared += 2
    assert compared == 256


@pytest.mark.parametrize("cn", CURVES)
def test_map_to_curve_both_branches_and_the_exceptional_case(probe, cn):
    got, _ = probe.records(cn, "map_to_curve")
    pairs = map_to_curve_cases(cn)
    assert len(pairs) == 10 + 1024 == len(got)
    assert pairs[0] == (0, 0) and pairs[4][1] == modulus(cn) - pairs[4][0] and pairs[3][0] == pairs[3][1]
    bad = []
    for (u0, u1), g in zip(pairs, got):
        x0, y0, x1, y1 = ints(g, 4)
        if ((x0, y0), (x1, y1)) != (K.map_to_curve_simple_swu(cn, u0), K.map_to_curve_simple_swu(cn, u1)):
            bad.append((hex(u0), hex(u1)))
    assert not bad, bad[:4]


@pytest.mark.parametrize("cn", CURVES)
def test_iso_add_generic_doubling_and_cancellation(probe, cn):
    got, _ = probe.records(cn, "iso_add")
    cases = iso_add_cases(cn)
    assert len(cases) == 64 + 24 + 512 == len(got)
    assert {k for _, _, k in cases[:64]} == {"generic", "double", "negate"}  # interleaved within the first wave
    bad, flagged = [], 0
    for (q0, q1, kind), g in zip(cases, got):
        sx, sy = ints(g, 2)
        flag = struct.unpack("<I", g[64:])[0]
        want = K.iso_add(cn, q0, q1)
        assert (want is None) == (kind == "negate")
        flagged += flag
        if (flag, sx, sy) != ((1, 0, 0) if want is None else (0, *want)):
            bad.append((kind, q0, q1))
    assert not bad, bad[:2]
    assert flagged == sum(k == "negate" for _, _, k in cases) == 21 + 8


@pytest.mark.parametrize("cn", CURVES)
def test_iso_map_images_and_the_kernel(probe, cn):
    got, _ = probe.records(cn, "iso_map")
    cases = iso_map_cases(cn)
    p = modulus(cn)
    n_sums = sum(k != "negate" for _, _, k in iso_add_cases(cn))
    assert len(cases) == n_sums + 3 + 4 == len(got)
    x0 = iso_kernel_x(cn)
    bad, identities, on_curve = [], 0, 0
    for ((x, y), on_iso), g in zip(cases, got):
        gx, gy = ints(g, 2)
        want = K.iso_map(cn, (x, y))
        assert on_iso == (y * y % p == g_iso(cn, x))
        if (gx, gy) != ((0, 0) if want is None else want):
            bad.append((hex(x), hex(y)))
        if (gx, gy) == (0, 0):
            identities += 1
            assert x == x0
        elif on_iso:  # the isogeny maps the isogenous curve onto y^2 = x^3 + 5; an input off the first has no reason to land on it
            assert gy * gy % p == (gx * gx * gx + 5) % p, (hex(x), hex(y))
            on_curve += 1
    assert not bad, bad[:4]
    assert identities == 3  # (x0, y) for the three ordinates, as iso_map returns None
    assert on_curve == sum(k for _, k in cases) >= n_sums + 2  # every input on the isogenous curve has its image on the curve


@pytest.mark.parametrize("cn", CURVES)
def test_hash_to_field_and_the_whole_point_under_three_tags(probe, cn):
    compared = 0
    for cfg, prefix, msg_len in tag_configs(cn):
        msgs = messages(cn, cfg, msg_len)
        assert len(msgs) == 64 and msgs[0] == bytes(msg_len) and msgs[1] == b"\xff" * msg_len
        params = dict(K.CK_DEFAULTS)  # the oracle takes its tag from its own dictionary: the strings the probe was given
        got_u, _ = probe.records(cn, "hash_to_field " + cfg)
        got_p, _ = probe.records(cn, "point " + cfg)
        assert len(got_u) == len(got_p) == 64
        for m, gu, gp in zip(msgs, got_u, got_p):
            assert ints(gu, 2) == K.hash_to_field(cn, prefix.encode(), m, params), (cfg, m.hex())
            want = K.hash_to_curve(cn, prefix.encode(), m, params)
            assert ints(gp, 2) == ((0, 0) if want is None else want), (cfg, m.hex())
            compared += 2
    assert compared == 3 * 64 * 2
