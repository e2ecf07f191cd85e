"""Model of the tile epilogue's tagged 32-bit row sort (tm_kernels.hip:
keep_lo_mask / tag_stage / tag_sort and the index gather of sort_classes), run
as plain Python on random rows -- no GPU.

Lane e of a W-wide group holds k32 = (code's high word | e), padding lanes
0xFFFFFFFF.  Every stage exchanges with lane ^ j and keeps min or max by a
per-stage constant lane mask; afterwards place e holds the entry that arrived
as number k32 & (W - 1).  The filter ids gathered that way must come out in
the order of a plain sort of the u64 entries (code | filter id), for every row
size 1..64 and every count of free low bits the path admits."""

import random

import pytest

KEY_MASK = 0xFFFFFFFF80000000


def keep_lo_mask(W, kk, j):
    m = 0
    for lane in range(64):
        e = lane & (W - 1)
        if ((e & j) == 0) == ((e & kk) == 0):
            m |= 1 << lane
    return m


def tag_sort_wave(k, W):
    """The W-wide network on all 64 lanes at once (64 / W rows side by side)."""
    k = list(k)
    kk = 2
    while kk <= W:
        j = kk >> 1
        while j > 0:
            m = keep_lo_mask(W, kk, j)
            other = [k[lane ^ j] for lane in range(64)]
            k = [min(k[lane], other[lane]) if (m >> lane) & 1 else max(k[lane], other[lane]) for lane in range(64)]
            j >>= 1
        kk <<= 1
    return k


def size_class(c):
    W = 2
    while W < c:
        W <<= 1
    return W


def random_row(rng, c, free):
    """c entries with distinct codes whose high words have `free` zero low bits
    (and bit 31 clear), in arrival order, with random filter ids."""
    his = set()
    while len(his) < c:
        top = rng.randint(0, 4) << 29                       # a code's top digit is 0..4
        hi = (top | rng.getrandbits(29)) & ~((1 << free) - 1)
        his.add(hi)
    his = list(his)
    rng.shuffle(his)
    return [(hi << 32) | rng.getrandbits(31) for hi in his]


def test_stage_masks_are_the_bitonic_rule():
    # kk == W: every lane of a row sorts upward, the mask is "lane's j bit clear"
    for W in (2, 4, 8, 16, 32, 64):
        j = W >> 1
        while j:
            assert keep_lo_mask(W, W, j) == sum(1 << lane for lane in range(64) if not lane & j)
            j >>= 1
    assert keep_lo_mask(4, 2, 1) == int("1001" * 16, 2)


@pytest.mark.parametrize("free", [5, 6, 7, 8])
def test_tagged_sort_orders_rows_like_a_u64_sort(free):
    rng = random.Random(100 + free)
    for c in range(1, 65):
        W = size_class(c)
        if W > (1 << free):
            continue                                         # this class takes the u64 network
        for _ in range(4):
            nrows = 64 // W
            rows = [random_row(rng, rng.randint(W // 2 + 1, W) if r else c, free) for r in range(nrows)]
            k = []
            for row in rows:
                for e in range(W):
                    k.append(((row[e] >> 32) | e) if e < len(row) else 0xFFFFFFFF)
            k = tag_sort_wave(k, W)
            for r, row in enumerate(rows):
                got = [row[k[r * W + e] & (W - 1)] & ~KEY_MASK for e in range(len(row))]
                assert got == [x & ~KEY_MASK for x in sorted(row)], (c, W, free)
                assert all(k[r * W + e] == 0xFFFFFFFF for e in range(len(row), W))


def test_free_bits_from_the_or_of_the_codes():
    """free = clamp(ctz(OR of the codes) - 32, 0, 8), computed in the kernel
    from bits 31..39: tz9 = ctz((or >> 31) | 0x200), free = max(tz9 - 1, 0)."""
    def kernel_free(kor):
        v = ((kor & KEY_MASK) >> 31) & 0xFFFFFFFF | 0x200
        tz9 = (v & -v).bit_length() - 1
        return tz9 - 1 if tz9 else 0

    def issue_free(kor):
        kor &= KEY_MASK
        tz = (kor & -kor).bit_length() - 1 if kor else 64
        return min(max(tz - 32, 0), 8)

    for bit in range(31, 64):
        assert kernel_free(1 << bit) == issue_free(1 << bit), bit
    rng = random.Random(3)
    for _ in range(2000):
        kor = rng.getrandbits(64) & KEY_MASK & ~((1 << rng.randint(31, 50)) - 1)
        assert kernel_free(kor) == issue_free(kor)
    assert kernel_free(0) == 8
