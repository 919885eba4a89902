"""The 3-byte rule codes of the coded rule-distance scan (five_hip_rule_distance_coded_ws), on the host: the multiply-and-shift
division of the field decode proved exhaustively, and a NumPy model of the dictionaries, the field packing and the lane-tiled
layout (include/frirl_hip.h) with round trips over random rule bases.  tests/test_hip_rule_distance_coded.py holds the pack
kernel to this model byte for byte."""
import numpy as np
import pytest

TILE = 2048                  # rules per tile: 256 threads x 2 rules x 4 column sets
TILE_BYTES = 3 * TILE


def ceil_log2(n):
    b = 0
    while (1 << b) < n:
        b += 1
    return b


def field_params(d):
    """(shift, mask, d_a, M) per field from the dictionary lengths, or None where the coded form does not apply."""
    nant = len(d)
    if nant > 5 or any(not 1 <= x <= 64 for x in d):
        return None
    fields, total = [], 0
    for k in range(0, nant, 2):
        da, db = d[k], (d[k + 1] if k + 1 < nant else 1)
        bits = ceil_log2(da * db)
        if bits > 12:
            return None
        fields.append((total, (1 << bits) - 1, da, -(-(1 << 18) // da)))
        total += bits
    return fields if total <= 24 else None


def dictionaries(uidx, nrules):
    """Per dimension: the sorted distinct 6-bit indices of the columns r < nrules[e] rounded up to the next even index."""
    E, nant, maxR = uidx.shape
    upto = np.minimum(nrules + (nrules & 1), maxR)
    live = np.arange(maxR)[None, :] < upto[:, None]
    out = []
    for k in range(nant):
        vals = np.unique((uidx[:, k, :] & 63)[live])
        out.append(vals if len(vals) else np.zeros(1, dtype=vals.dtype))       # an empty dictionary counts as one entry
    return out


def encode(uidx, nrules, dicts, fields):
    """codes[e][r] (uint32, < 2^24); 0 in the columns the dictionaries do not cover."""
    E, nant, maxR = uidx.shape
    upto = np.minimum(nrules + (nrules & 1), maxR)
    live = np.arange(maxR)[None, :] < upto[:, None]
    digits = [np.searchsorted(dicts[k], uidx[:, k, :] & 63).astype(np.uint32) for k in range(nant)]
    codes = np.zeros((E, maxR), dtype=np.uint32)
    for f, (shift, mask, da, _) in enumerate(fields):
        v = digits[2 * f].copy()
        if 2 * f + 1 < nant:
            v += digits[2 * f + 1] * np.uint32(da)
        codes |= np.where(live, v, 0).astype(np.uint32) << np.uint32(shift)
    return codes


def decode(codes, nant, fields):
    """digits[k][...] from codes with the kernel's arithmetic: j_b = (v * M) >> 18, j_a = v - j_b * d_a."""
    digits = []
    for f, (shift, mask, da, M) in enumerate(fields):
        v = (codes >> np.uint32(shift)) & np.uint32(mask)
        if 2 * f + 1 < nant:
            jb = (v * np.uint32(M)) >> np.uint32(18)
            digits += [v - jb * np.uint32(da), jb]
        else:
            digits.append(v)
    return digits


def tile_layout(codes):
    """The lane-tiled byte image of codes[E][maxR]: per environment ceil(maxR / 2048) tiles of 6144 bytes; thread t of a tile owns
    rules 2t + p + 512 j, its codes in the order 2j + p are one 24-byte little-endian string, piece m at tile + 2048 m + 8 t."""
    E, maxR = codes.shape
    tpe = -(-maxR // TILE)
    pad = np.zeros((E, tpe * TILE), dtype=np.uint32)
    pad[:, :maxR] = codes
    c = pad.reshape(E, tpe, 4, 256, 2)                          # [e][tile][j][t][p]
    c = c.transpose(0, 1, 3, 2, 4).reshape(E, tpe, 256, 8)      # [e][tile][t][2j + p]
    b = np.stack([(c >> (8 * i)) & 0xFF for i in range(3)], axis=-1).astype(np.uint8)      # [e][tile][t][code][byte]
    s = b.reshape(E, tpe, 256, 3, 8)                            # the 24-byte string as three pieces
    return np.ascontiguousarray(s.transpose(0, 1, 3, 2, 4)).reshape(E, tpe * TILE_BYTES)


def untile(image, maxR):
    E = image.shape[0]
    tpe = -(-maxR // TILE)
    s = image.reshape(E, tpe, 3, 256, 8).transpose(0, 1, 3, 2, 4).reshape(E, tpe, 256, 8, 3).astype(np.uint32)
    c = s[..., 0] | s[..., 1] << 8 | s[..., 2] << 16
    return c.reshape(E, tpe, 256, 4, 2).transpose(0, 1, 3, 2, 4).reshape(E, tpe * TILE)[:, :maxR]


def test_magic_division_exhaustive():
    """j_b = (v * M) >> 18 with M = ceil(2^18 / d) is v // d for every d <= 64 and v < 4096, within 24-bit operands and a 32-bit product."""
    v = np.arange(4096, dtype=np.uint64)
    for d in range(1, 65):
        M = -(-(1 << 18) // d)
        assert M < (1 << 24) and 4095 * M < (1 << 32)
        q = (v * np.uint64(M)) >> np.uint64(18)
        assert (q == v // np.uint64(d)).all(), d
        assert (v - q * np.uint64(d) == v % np.uint64(d)).all(), d


def test_shift_17_is_not_a_division():
    """The mutation `>> 17` in the decode is caught by the same sweep."""
    v = np.arange(4096, dtype=np.uint64)
    assert all((((v * np.uint64(-(-(1 << 18) // d))) >> np.uint64(17)) != v // np.uint64(d)).any() for d in range(1, 65))


def test_field_params():
    f = field_params([41, 41, 41, 41, 3])                       # cfg4: 11 + 11 + 2 = 24 bits
    assert [(s, m) for s, m, _, _ in f] == [(0, 2047), (11, 2047), (22, 3)]
    assert f[0][2] == 41 and f[0][3] == 6394
    f = field_params([41, 41, 3])                               # cfg2: 11 + 2
    assert [(s, m) for s, m, _, _ in f] == [(0, 2047), (11, 3)]
    assert field_params([41] * 5) is None                       # 11 + 11 + 6 = 28 bits
    assert field_params([64, 64]) is not None and field_params([64, 64, 64, 64, 1]) is not None         # 12 + 12 + 0
    assert field_params([64, 64, 64, 64, 2]) is None
    assert field_params([1]) == [(0, 0, 1, 1 << 18)]
    assert field_params([41] * 6) is None


def random_base(rng, nant, maxR, E, sizes):
    """Rule bases whose dimension k uses a random subset of sizes[k] indices out of 64; ragged rule counts."""
    uidx = np.zeros((E, nant, maxR), dtype=np.uint16)
    for k in range(nant):
        pool = np.sort(rng.choice(64, size=sizes[k], replace=False))
        uidx[:, k, :] = pool[rng.integers(0, sizes[k], size=(E, maxR))]
    nrules = rng.integers(0, maxR + 1, size=E).astype(np.int32)
    nrules[0] = maxR
    return uidx, nrules


@pytest.mark.parametrize("sizes,maxR", [((41, 41, 41, 41, 3), 4098), ((41, 41, 3), 2050), ((64, 64), 2048), ((7,), 10), ((64, 64, 64, 64, 1), 600),
                                         ((1, 1, 1), 6), ((5, 64, 33, 2), 4100)])
def test_round_trip(sizes, maxR):
    rng = np.random.default_rng(sum(sizes) + maxR)
    nant, E = len(sizes), 5
    uidx, nrules = random_base(rng, nant, maxR, E, sizes)
    dicts = dictionaries(uidx, nrules)
    fields = field_params([len(x) for x in dicts])
    assert fields is not None
    codes = encode(uidx, nrules, dicts, fields)
    assert (codes < (1 << 24)).all()
    image = tile_layout(codes)
    assert image.shape == (E, -(-maxR // TILE) * TILE_BYTES)
    back = untile(image, maxR)
    assert (back == codes).all()
    digits = decode(back, nant, fields)
    upto = np.minimum(nrules + (nrules & 1), maxR)
    for e in range(E):
        for k in range(nant):
            assert (dicts[k][digits[k][e, :upto[e]]] == (uidx[e, k, :upto[e]] & 63)).all(), (e, k)
            assert (digits[k][e, upto[e]:] == 0).all(), (e, k)


def test_layout_addresses():
    """Piece m of thread t of tile c lies at c * 6144 + 2048 m + 8 t and holds bytes 8m .. 8m + 7 of the string of codes 2j + p."""
    maxR = 4098
    codes = ((np.arange(maxR, dtype=np.uint64) * 2654435761 >> 8) & 0xFFFFFF)[None, :].astype(np.uint32)
    image = tile_layout(codes)[0]
    for c, t in ((0, 0), (0, 255), (1, 17), (2, 0)):
        rules = [c * TILE + 2 * t + p + 512 * j for j in range(4) for p in range(2)]
        string = b"".join(int(codes[0, r] if r < maxR else 0).to_bytes(3, "little") for r in rules)
        for m in range(3):
            at = c * TILE_BYTES + 2048 * m + 8 * t
            assert image[at:at + 8].tobytes() == string[8 * m:8 * m + 8], (c, t, m)
