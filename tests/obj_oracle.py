"""The OBJ text contract of include/sdfa_obj.h restated in integer Python / numpy: float32 bit patterns -> the "{:.6f}" text
Python prints for them, without any floating point, and the vertex / face blocks built from it.  The test data the CPU and
GPU tests share (edge list, exact ties, in-domain bit patterns, N(0, 0.1)) is generated here from fixed seeds."""
import numpy as np

MAX_LINE_BYTES = 59

EDGES = np.array([0.0, -0.0, 1e-7, -1e-7, 5e-7, 0.9999995, 0.99999949, 9.9999995, 999999.94, 1e-45, 1.17549435e-38,
                  2147483520.0, -2147483520.0, 16777216.0, 8388608.5], np.float32)


def with_neighbours(x):
    x = np.atleast_1d(np.asarray(x, np.float32))
    return np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])


def edge_values():
    """The edge list, with both float32 neighbours of 5e-7 (the smallest value that can round up to 0.000001)."""
    return np.concatenate([EDGES, with_neighbours(np.float32(5e-7))[1:]])


def tie_values():
    """Every j / 128 for |j| <= 4001 with both neighbours: odd j are exact ties of the sixth decimal."""
    return with_neighbours((np.arange(-4001, 4002) / 128.0).astype(np.float32))


def domain_patterns(n, seed):
    """Random sign, exponent field uniform over 0 .. 157, random fraction: the whole domain, denormals included."""
    rs = np.random.RandomState(seed)
    bits = (rs.randint(0, 2, n).astype(np.uint32) << 31) | (rs.randint(0, 158, n).astype(np.uint32) << 23) | \
        rs.randint(0, 1 << 23, n).astype(np.uint32)
    return bits.view(np.float32)


def normal_values(n, seed):
    return np.random.RandomState(seed).normal(0, 0.1, n).astype(np.float32)


def in_domain(x):
    bits = np.asarray(x, np.float32).view(np.uint32)
    return ((bits >> 23) & 0xff) < 158


def scaled(bits):
    """(sign, Q): Q = |x| * 10^6 rounded half to even, from the float32 bit pattern (a Python int)."""
    s, E, M = bits >> 31, (bits >> 23) & 0xff, bits & 0x7fffff
    assert E < 158, "outside the domain"
    m, e = (M, -149) if E == 0 else (M | 1 << 23, E - 150)
    N, k = m * 15625, e + 6
    if k >= 0:
        return s, N << k
    sh = -k
    if sh >= 40:
        return s, 0
    Q, rem, half = N >> sh, N & ((1 << sh) - 1), 1 << (sh - 1)
    if rem > half or (rem == half and Q & 1):
        Q += 1
    return s, Q


def number(bits):
    s, Q = scaled(int(bits))
    return ("-" if s else "") + "%d.%06d" % (Q // 1000000, Q % 1000000)


def numbers(x):
    """list of the texts of a float32 array's elements"""
    return [number(b) for b in np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32).tolist()]


def vertex_block(verts):
    t = numbers(verts)
    return "".join("v %s %s %s\n" % (t[i], t[i + 1], t[i + 2]) for i in range(0, len(t), 3)).encode()


def face_block(faces):
    return "".join("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in np.asarray(faces).reshape(-1, 3).tolist()).encode()
