"""The field decode of the coded rule-distance scan (cd_rule_sq in csrc/five_rule_distance.hip) in byte offsets, on the host: a NumPy
model of the instructions the scan issues per pair field -- operands cut to 24 bits and products wrapped to 32 as v_mul_u32_u24 and
v_mad_i32_i24 have them -- held to (v % d_a, v // d_a) for every dictionary length pair the coded form admits (d_a, d_b in 1..64,
d_a * d_b <= 4096; the shipped shapes have d_a * d_b <= 2048), every field value v below 2^bits, valid or not, and every shift the field
can have in a 24-bit code, with the other bits of the word set at random.  The unpacking of a lane's three 8-byte pieces into eight
codes at bit 3 is modelled too."""
import numpy as np

from tests.test_rd_codes_host import ceil_log2

M32 = np.uint64(0xFFFFFFFF)
M24 = np.uint64(0xFFFFFF)
QSHIFT = 18                  # the magic's basis: magic = ceil(2^18 / d_a)
QMASK = 127 << 3             # RD_CD_Q8


def u(x):
    return np.uint64(x)


def sext24(x):
    """The low 24 bits of x as a signed integer (int64)."""
    x = (x & M24).astype(np.int64)
    return np.where(x >= 1 << 23, x - (1 << 24), x)


def mul_u32_u24(a, b):
    return ((a & M24) * (b & M24)) & M32


def mad_i32_i24(a, b, c):
    return ((sext24(a) * sext24(b) + c.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint64)


def decode_pair8(code8, shift, bits, da, qshift=QSHIFT, qmask=QMASK):
    """(8 j_a, 8 j_b) of the pair field at `shift` of codes held at bit 3 of 32-bit words, with the scan's constants: mask8 = mask << 3,
    magic = ceil(2^18 / d_a), -d_a as a 32-bit word."""
    mask8 = u(((1 << bits) - 1) << 3)
    magic = u(-(-(1 << 18) // da))
    negda = u((-da) & 0xFFFFFFFF)
    v8 = (code8 >> u(shift)) & mask8
    jb8 = (mul_u32_u24(v8, magic) >> u(qshift)) & u(qmask)
    ja8 = mad_i32_i24(jb8, negda, v8)
    return ja8, jb8


def words_with_field(rng, v, shift, bits):
    """32-bit words holding v at bit shift + 3 and random bits everywhere else (one row per shift)."""
    junk = rng.integers(0, 1 << 32, size=np.broadcast(v, shift).shape, dtype=np.uint64)
    field = u((1 << bits) - 1) << (shift + u(3))
    return ((junk & ~field) | (v << (shift + u(3)))) & M32


def cases():
    """(d_a, bits) of every pair the coded form admits: bits = ceil(log2(d_a * d_b)) <= 12."""
    for da in range(1, 65):
        for bits in sorted({ceil_log2(da * db) for db in range(1, 65)}):
            if bits <= 12:
                yield da, bits


def sweep(qshift=QSHIFT, qmask=QMASK):
    """The number of (d_a, bits) cases in which the model differs from (v % d_a, v // d_a) somewhere."""
    rng = np.random.default_rng(5)
    bad = n = 0
    for da, bits in cases():
        v = np.arange(1 << bits, dtype=np.uint64)[None, :]
        shift = np.arange(0, 24 - bits + 1, dtype=np.uint64)[:, None]
        ja8, jb8 = decode_pair8(words_with_field(rng, v, shift, bits), shift, bits, da, qshift, qmask)
        ok = (ja8 == 8 * (v % u(da))).all() and (jb8 == 8 * (v // u(da))).all()
        bad += not ok
        n += 1
    return bad, n


def test_pair_decode_exhaustive():
    bad, n = sweep()
    assert n > 64 * 6 and bad == 0, bad


def test_operand_ranges():
    """What keeps the products inside 24 x 24 -> 32 bits: v8 < 2^15, magic <= 2^18, and v8 * magic < 2^32 because 2^bits < 2 d_a d_b."""
    for da, bits in cases():
        magic = -(-(1 << 18) // da)
        assert magic <= 1 << 18 and ((1 << bits) - 1) * 8 < 1 << 15
        assert ((1 << bits) - 1) * 8 * magic < 1 << 32, (da, bits)
        assert ((1 << bits) - 1) // da < 128                                     # the quotient of an invalid v still fits RD_CD_Q8
        assert 8 * 127 * da < 1 << 23


def test_wrong_constants_fail():
    """Mutations of the constants are caught by the same sweep: the quotient shifted by 21 (a digit, not a byte offset), by 17, and a
    quotient mask that keeps a fraction bit."""
    for kw in ({"qshift": 21}, {"qshift": 17}, {"qmask": 255 << 2}):
        bad, n = sweep(**kw)
        assert bad > n // 2, (kw, bad, n)


def test_single_field():
    """An odd last dimension: 8 v is the shift and the mask."""
    rng = np.random.default_rng(6)
    for bits in range(0, 7):
        v = np.arange(1 << bits, dtype=np.uint64)[None, :]
        shift = np.arange(0, 24 - bits + 1, dtype=np.uint64)[:, None]
        w = words_with_field(rng, v, shift, bits)
        assert (((w >> shift) & u(((1 << bits) - 1) << 3)) == 8 * v).all()


def alignbit(hi, lo, s):
    return (((hi << u(32)) | lo) >> u(s)) & M32


def test_unpack_to_bit_3():
    """A lane's 24-byte string of eight codes as three little-endian 8-byte pieces (x = low word): the scan's eight shifts put code i at
    bit 3 of word i."""
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 1 << 24, size=(1000, 8), dtype=np.uint64)
    codes[0], codes[1] = 0xFFFFFF, 0
    string = sum(codes[:, i].astype(object) << (24 * i) for i in range(8))                  # Python integers: 192 bits
    word = lambda i: np.array([(int(s) >> (32 * i)) & 0xFFFFFFFF for s in string], dtype=np.uint64)      # noqa: E731
    w0x, w0y, w1x, w1y, w2x, w2y = (word(i) for i in range(6))
    code8 = [(w0x << u(3)) & M32, alignbit(w0y, w0x, 21), alignbit(w1x, w0y, 13), w1x >> u(5),
             (w1y << u(3)) & M32, alignbit(w2x, w1y, 21), alignbit(w2y, w2x, 13), w2y >> u(5)]
    for i in range(8):
        assert (((code8[i] >> u(3)) & M24) == codes[:, i]).all(), i
