"""The seams of dcn_anchor_map_reference_blocks and its kernels (blocks.hip), on the two records of
tests/test_gpu_pileup_seams.py (3989 and 1777 bases, the second beginning mid-word of the store: its position p is slot
p + 1 of a whole-record call, counted from the aligned start).  Counters are set by hand: reference-exact reads laid over
chosen intervals (`cover`), reads whose odd bases are of low quality (`alternate`), and the columns of
tests/test_gpu_genotype_seams.py.  One scene is piled up once per module; what a case wants to hit is asserted on the
model (tests/_blocks_worker.py) first, then cls and every block are compared with it.  Exact throughout."""
import ctypes as C

import numpy as np
import pytest

import _blocks_worker as BW
import _genotype_worker as GW
import _pileup_worker as PW
import _verify_worker as VW
from test_gpu_genotype_seams import column
from test_gpu_pileup_qual_seams import QCase, run
from test_gpu_pileup_seams import LEN0, LEN1, make_records

pytestmark = pytest.mark.gpu

D = dict(GW.DEFAULTS)
LOOSE = dict(D, min_gq=0)           # every position of depth 3 and more with a reference genotype is REF
EDGES = BW.DEFAULT_EDGES
FIFTEEN = tuple(range(6, 96, 6))    # 6, 12 .. 90


def cover(c, R, a, b, k, q=30, tile=150):
    """k reference-exact reads over every base of [a, b), strands alternating"""
    for lo in range(a, b, tile):
        hi = min(b, lo + tile)
        S = c.records[R][lo:hi].upper().replace(b"N", b"A")
        for i in range(k):
            c.put(S, q, R, lo, hi, rev=i % 2)


def alternate(c, R, a, b, k, tile=150):
    """k reference-exact reads over [a, b) whose bases at odd positions are of quality 3: under min_base_qual they count as N,
    so D is k at the even positions and 0 at the odd ones, with depth k at both"""
    for lo in range(a, b, tile):
        hi = min(b, lo + tile)
        S = c.records[R][lo:hi].upper().replace(b"N", b"A")
        for i in range(k):
            c.put(S, [3 if p & 1 else 30 for p in range(lo, hi)], R, lo, hi, rev=i % 2)


# where the classes change: record 0 begins at store base 0, record 1 at 3989, so a position p of record 1 is slot p + 1
CHANGES0 = [256, 600, 701, 802, 903, 1024]   # a wave's edge; 0, 1, 2, 3 mod 4; a workgroup's edge
CHANGES1 = [203, 255, 1500, 1601, 1702]      # slots 204 (0 mod 4), 256 (a wave's edge), 1501 (1), 1602 (2), 1703 (3)
ALT1 = (301, 1500)                           # record 1: alternating, over the workgroup's edge at position 1023
BIG0 = (1060, 3100)                          # record 0: one block over workgroups 1, 2 and 3 of a whole-record call
N_ONLY, DEL_ONLY, HET, GQ30, GQ99 = 3200, 3300, 3400, 3500, 3600


@pytest.fixture(scope="module")
def env(dcn, oracle):
    records = make_records()
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_qualities()
    placer = dcn.Placer(amap, max_batch_bases=1 << 22, max_batch_reads=1 << 16)
    yield dcn, oracle, records, amap, placer
    placer.close()
    amap.close()


@pytest.fixture(scope="module")
def scene(env):
    """the one pile-up of this module -> (counts, sums) of both records, as the CPU model piles them"""
    dcn, O, records, amap, placer = env
    c = QCase(dcn, records, 240)
    # record 0
    cover(c, 0, 100, 256, 8)
    cover(c, 0, 256, 600, 16)
    cover(c, 0, 600, 701, 1)
    cover(c, 0, 701, 802, 8)
    cover(c, 0, 903, 1024, 8)
    cover(c, 0, 1024, 1060, 1)
    cover(c, 0, BIG0[0], BIG0[1], 4)
    cover(c, 0, BIG0[0], 2500, 2)
    cover(c, 0, 2600, BIG0[1], 2)
    cover(c, 0, 3080, BIG0[1], 14)
    column(c, 0, 1200, [(0, 30)] * 3 + [(1, 20)])        # nine reference bases and one other: the smallest GQ of the block
    column(c, 0, N_ONLY, [(0, 3)] * 4)
    column(c, 0, DEL_ONLY, [(None, 0)] * 4)
    column(c, 0, HET, [(0, 30)] * 5 + [(1, 30)] * 5)     # QUAL 143
    column(c, 0, GQ30, [(0, 30)] * 10)
    column(c, 0, GQ99, [(0, 30)] * 40)
    cover(c, 0, 3900, LEN0, 8)
    # record 1
    cover(c, 1, 60, 102, 8)                              # its NNN is 100 .. 102: two covered, one not
    cover(c, 1, 150, 203, 8)
    cover(c, 1, 203, 255, 1)
    cover(c, 1, 255, ALT1[0], 8)
    alternate(c, 1, ALT1[0], ALT1[1], 8)
    cover(c, 1, 1500, 1601, 8)
    cover(c, 1, 1702, LEN1, 8)
    counts, sums, _, _ = run(c, amap, placer, O)
    return counts, sums


def whole(env, scene, R, breaks=(), edges=EDGES, **params):
    dcn, O, records, amap, placer = env
    return BW.assert_range(amap, scene[0][R], scene[1][R], records[R], R, 0, None, breaks, edges, **params)


def block_at(blocks, p):
    return next(b for b in blocks if b[0] <= p < b[0] + b[1])


def test_class_changes_at_kernel_seams(env, scene):
    """a class change at slots 0, 1, 2 and 3 mod 4, across a wave's edge (slot 256) and across a workgroup's (slot 1024), on
    both records"""
    for R, changes, pad in ((0, CHANGES0, 0), (1, CHANGES1, 1)):
        cls, blocks = whole(env, scene, R, **D)
        assert {(p + pad) % 4 for p in changes} == {0, 1, 2, 3} and any((p + pad) == 256 for p in changes)
        for p in changes:
            assert cls[p - 1] != cls[p] and BW.VARIANT not in (cls[p - 1], cls[p]), (R, p)
            assert any(b[0] == p for b in blocks) and any(b[0] + b[1] == p for b in blocks)
    cls1, _ = whole(env, scene, 1, **D)
    assert 1024 in CHANGES0 and cls1[1022] != cls1[1023] != cls1[1024]  # record 1: slot 1024 is position 1023, inside the alternation


def test_a_block_over_three_workgroups(env, scene):
    """one block over workgroups 1, 2 and 3: its smallest GQ lies in the first, its smallest depth in the middle one, its
    largest in the last, so every number of the record is combined across workgroups"""
    dcn, O, records, amap, placer = env
    cls, blocks = whole(env, scene, 0, edges=(), **LOOSE)
    b = block_at(blocks, 2000)
    assert (b[0], b[0] + b[1]) == BIG0 and b[2] == BW.REF and b[0] < 2048 and b[0] + b[1] > 3072
    per = [BW.classify(scene[0][0][p], scene[1][0][p], PW.column(records[0][p]), False, (), **LOOSE) for p in range(*BIG0)]
    gq, depth = [x[1] for x in per], [x[2] for x in per]
    at = lambda values, v: {BIG0[0] + i for i, x in enumerate(values) if x == v}
    assert at(gq, min(gq)) == {1200} and b[3] == min(gq) == 5
    assert all(2048 <= p < 3072 for p in at(depth, min(depth))) and b[4] == min(depth) == 4
    assert all(p >= 3072 for p in at(depth, max(depth))) and b[5] == max(depth) == 20 and b[6] == sum(depth)


def test_alternating_classes(env, scene):
    """1,199 consecutive positions whose class changes at every one: every position a head, over a workgroup's edge"""
    cls, blocks = whole(env, scene, 1, **D)
    a, b = ALT1
    assert all(cls[p] != cls[p + 1] for p in range(a, b - 1)) and set(cls[a:b].tolist()) == {BW.UNCALLED, BW.REF + 1}
    inside = [x for x in blocks if a <= x[0] < b]
    assert len(inside) == b - a > 1024 and all(x[1] == 1 for x in inside)
    dcn, O, records, amap, placer = env
    for start, n in ((a, b - a), (a + 1, 1025), (a + 2, 1024), (a + 3, 1023)):  # every position of a range a block: capacity = n
        want = BW.assert_range(amap, scene[0][1], scene[1][1], records[1], 1, start, n, **D)
        assert len(want[1]) == n


def test_variant_placement(env, scene):
    """VARIANT first and last of the range, two adjacent, and one that splits a run of one class into two blocks"""
    dcn, O, records, amap, placer = env
    start, n = 300, 250
    breaks = [start, start + n - 1, 400, 401, 450]
    cls, blocks = BW.assert_range(amap, scene[0][0], scene[1][0], records[0], 0, start, n, breaks, **D)
    assert set(cls.tolist()) == {BW.VARIANT, BW.REF + 2}
    assert [(b[0], b[1]) for b in blocks] == [(301, 99), (402, 48), (451, 98)] and len({b[2] for b in blocks}) == 1
    # a G7 site does the same without a break
    prm = dict(D, min_qual=143)
    cls, blocks = BW.assert_range(amap, scene[0][0], scene[1][0], records[0], 0, HET - 10, 20, **prm)
    assert cls[10] == BW.VARIANT and [(b[0], b[1]) for b in blocks] == [(HET - 10, 10), (HET + 1, 9)] and blocks[0][2] == blocks[1][2]


def test_breaks(env, scene):
    """breaks duplicated and unordered, on a G7 site, at both ends of the range; one outside: an error, nothing written"""
    dcn, O, records, amap, placer = env
    N = dcn._native
    prm = dict(D, min_qual=143)
    start, n = HET - 15, 40
    for breaks in ([HET], [start + n - 1, start, HET, start, HET + 1, start + n - 1, HET + 1], [start + 5] * 300):
        cls, blocks = BW.assert_range(amap, scene[0][0], scene[1][0], records[0], 0, start, n, breaks, **prm)
        assert cls[HET - start] == BW.VARIANT
    for R in (0, 1):
        whole(env, scene, R, breaks=[0, len(records[R]) - 1], **D)
    p = N.BlockParams(2, 3, 20, 20, 477, 301, 0, 0, (C.c_uint8 * 16)())
    for bad, index in (([start, start + n], 1), ([start - 1], 0), ([start + 1, 2 ** 63, start - 1], 1)):
        brk = np.array(bad, np.uint64)
        cls, blocks, count = np.full(n, 77, np.uint8), np.full(8, 0x55, np.uint8).repeat(40), C.c_uint64(12345)
        rc = N.lib().dcn_anchor_map_reference_blocks(amap._h, C.byref(p), 0, start, n, brk.ctypes.data_as(C.c_void_p), len(brk),
                                                     cls.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p), 8, C.byref(count))
        assert rc == N.DCN_ERR_ARG and ("breaks[%d]" % index).encode() in N.lib().dcn_last_error()
        assert (cls == 77).all() and (blocks == 0x55).all() and count.value == 12345


def test_every_branch_of_the_class(env, scene):
    """rule B2 branch by branch: coverage by N only and by DEL only; an invalid reference base with and without coverage; a
    called non-reference position under min_qual; GQ at an edge, one under and one over it; no edge and fifteen; edge 99
    with GQ 99; both ploidies"""
    dcn, O, records, amap, placer = env
    counts, sums = scene
    cls, _ = whole(env, scene, 0, **D)
    p_del = DEL_ONLY - 20 + int(np.argmax(counts[0][DEL_ONLY - 20:DEL_ONLY + 20, PW.DEL]))
    for p, col in ((N_ONLY, PW.N), (p_del, PW.DEL)):
        assert counts[0][p][col] == 4 and counts[0][p][:4].sum() == 0 and cls[p] == BW.UNCALLED
    assert not counts[0][50].any() and cls[50] == BW.NO_COVERAGE
    cls1, _ = whole(env, scene, 1, **D)
    assert records[1][100:103] == b"NNN" and counts[1][100][:4].sum() == counts[1][101][:4].sum() == 8 and not counts[1][102].any()
    assert cls1[99] == BW.REF + 1 and cls1[100] == cls1[101] == BW.UNCALLED and cls1[102] == BW.NO_COVERAGE
    # a called heterozygote of QUAL 143: a site at min_qual 143, no site and no reference genotype at 144
    assert whole(env, scene, 0, **dict(D, min_qual=143))[0][HET] == BW.VARIANT
    assert whole(env, scene, 0, **dict(D, min_qual=144))[0][HET] == BW.UNCALLED
    # GQ 30 against an edge at 29, 30 and 31; GQ 99 against an edge at 99; no edge; fifteen edges
    assert BW.classify(counts[0][GQ30], sums[0][GQ30], PW.column(records[0][GQ30]), **D)[1] == 30
    assert BW.classify(counts[0][GQ99], sums[0][GQ99], PW.column(records[0][GQ99]), **D)[1] == 99
    for edges, band30, band99 in (((29,), 1, 1), ((30,), 1, 1), ((31,), 0, 1), ((99,), 0, 1), ((), 0, 0), (FIFTEEN, 5, 15), ((1, 30, 98, 99), 2, 4)):
        for ploidy in (1, 2):  # (a window with both columns; whole records below)
            got, _ = BW.assert_range(amap, counts[0], sums[0], records[0], 0, GQ30 - 50, 200, (), edges, **dict(D, ploidy=ploidy))
            if ploidy == 2:
                assert got[50] == BW.REF + band30 and got[GQ99 - GQ30 + 50] == BW.REF + band99, edges
    for R in (0, 1):
        whole(env, scene, R, edges=FIFTEEN, **LOOSE)
        whole(env, scene, R, edges=(), **dict(D, ploidy=1))
    haploid = set(whole(env, scene, 0, **dict(D, ploidy=1))[0].tolist())
    assert haploid >= {BW.NO_COVERAGE, BW.UNCALLED, BW.REF + 5}  # (a haploid reference call is sure: GQ 99)
    assert len(FIFTEEN) == 15


def test_ranges_and_cuts(env, scene):
    """n = 1, the last position, n = 0; every cut in a window around a class change, at every residue of the cut mod 4:
    the two halves, merged, are the whole (rule B7)"""
    dcn, O, records, amap, placer = env
    counts, sums = scene
    for R, length in ((0, LEN0), (1, LEN1)):
        for start in (0, 1, 2, 3, 600, 1023, 1024, length - 1):
            want = BW.assert_range(amap, counts[R], sums[R], records[R], R, start, 1, **D)
            assert len(want[1]) == 1
        BW.assert_range(amap, counts[R], sums[R], records[R], R, length - 1, 1, [length - 1], **D)
        for start in (0, 5, length):
            cls, blocks = amap.reference_blocks(R, start, 0)
            assert len(cls) == 0 and len(blocks) == 0
    for R, change, lo, hi in ((0, 600, 500, 760), (1, 255, 180, 330)):
        breaks = [lo + 20, change + 30]
        _, want = BW.assert_range(amap, counts[R], sums[R], records[R], R, lo, hi - lo, breaks, **D)
        cuts = list(range(change - 6, change + 7)) + [lo, lo + 1, hi - 1, hi, lo + 20, lo + 21]
        assert {m % 4 for m in cuts} == {0, 1, 2, 3}
        for m in cuts:
            halves = []
            for a, b in ((lo, m), (m, hi)):
                _, part = BW.assert_range(amap, counts[R], sums[R], records[R], R, a, b - a, [x for x in breaks if a <= x < b], **D)
                halves += part
            merged = dcn.merge_blocks(BW.to_array(dcn.REFERENCE_BLOCK_DTYPE, halves))
            assert BW.device_blocks(merged) == want == BW.merge(halves), (R, m)


def test_capacity_protocol(env, scene):
    """NULL with capacity 0 asks for the count; one too few leaves cls complete and writes no block; exact fits"""
    dcn, O, records, amap, placer = env
    N = dcn._native
    start, n = 200, 900
    want_cls, want = BW.blocks_range(scene[0][0], scene[1][0], records[0], start, n, **D)
    assert len(want) >= 5
    p = N.BlockParams(2, 3, 20, 20, 477, 301, 5, 0, (C.c_uint8 * 16)(*EDGES))

    def call(capacity, null=False):
        cls, blocks, count = np.full(n, 77, np.uint8), np.full(len(want) + 1, 0x55, np.uint8).repeat(40), C.c_uint64(12345)
        rc = N.lib().dcn_anchor_map_reference_blocks(amap._h, C.byref(p), 0, start, n, None, 0, cls.ctypes.data_as(C.c_void_p),
                                                     None if null else blocks.ctypes.data_as(C.c_void_p), capacity, C.byref(count))
        return rc, cls, blocks, count.value

    for capacity, null in ((0, True), (len(want) - 1, False)):
        rc, cls, blocks, count = call(capacity, null)
        assert rc == N.DCN_ERR_CAPACITY and count == len(want) and np.array_equal(cls, want_cls) and (blocks == 0x55).all()
    rc, cls, blocks, count = call(len(want))
    assert rc == N.DCN_OK and count == len(want) and np.array_equal(cls, want_cls) and (blocks[len(want) * 40:] == 0x55).all()
    assert BW.device_blocks(blocks[:len(want) * 40].view(dcn.REFERENCE_BLOCK_DTYPE)) == want


def test_repeat_calls(env, scene):
    """a second call on the same map with other parameters sees nothing of the first, and the first again gives the first"""
    first = whole(env, scene, 0, **D)
    second = whole(env, scene, 0, breaks=[700, 2000], edges=(10, 25), **dict(LOOSE, ploidy=1, min_depth=9))
    again = whole(env, scene, 0, **D)
    assert first[1] == again[1] and first[1] != second[1] and np.array_equal(first[0], again[0])


def test_the_order_of_the_errors_by_behaviour(env, scene, oracle):
    """two errors at once, the earlier check's message wins: the parameters before the map's state, the map's state before the
    range, the range before n_blocks NULL, n_blocks NULL before a break outside the range; nothing is written"""
    dcn, O, records, amap, placer = env
    N, L = dcn._native, dcn._native.lib()
    good = N.BlockParams(2, 3, 20, 20, 477, 301, 0, 0, (C.c_uint8 * 16)())
    bad_edges = N.BlockParams(2, 3, 20, 20, 477, 301, 1, 0, (C.c_uint8 * 16)(100))
    outside = np.array([LEN0 + 5], np.uint64)
    inside = np.array([10], np.uint64)
    plain = VW.build_map(oracle, dcn, records)  # a pileup without quality sums
    plain.pileup_enable()
    bare = VW.build_map(oracle, dcn, records)   # no pileup at all
    try:
        def call(m, p, record, start, n, brk, with_count=True):
            cls, count = np.full(64, 77, np.uint8), C.c_uint64(12345)
            rc = L.dcn_anchor_map_reference_blocks(m._h, C.byref(p), record, start, n, brk.ctypes.data_as(C.c_void_p), len(brk),
                                                   cls.ctypes.data_as(C.c_void_p), None, 0, C.byref(count) if with_count else None)
            assert rc == N.DCN_ERR_ARG and (cls == 77).all() and count.value == 12345
            return L.dcn_last_error()

        assert b"params.edges[0] must be 1..99" in call(bare, bad_edges, 9, LEN0, 64, outside, False)      # 2 before 3, 4, 5, 6
        assert b"the map has no pileup" in call(bare, good, 9, LEN0, 64, outside, False)                  # 3 before 4, 5, 6
        sums_error = call(plain, good, 9, LEN0, 64, outside, False)
        assert b"the map keeps no quality sums" in sums_error and b"n_blocks" not in sums_error and b"breaks[" not in sums_error  # 3 (the sums') before 4, 5, 6
        for record, start, n in ((9, 0, 64), (0, LEN0 - 10, 64), (0, LEN0, 1)):                        # 4 before 5 and 6
            message = call(amap, good, record, start, n, outside, False)
            assert message.startswith(b"reference blocks") and b"n_blocks" not in message and b"breaks[" not in message, message
            message = call(amap, good, record, start, n, outside)
            assert message.startswith(b"reference blocks") and b"breaks[" not in message, message
        assert b"n_blocks is NULL" in call(amap, good, 0, 0, 64, outside, False)                           # 5 before 6
        assert b"n_blocks is NULL" in call(amap, good, 0, 0, 64, inside, False)
        assert b"breaks[0] = %d is outside the range [0, 64)" % (LEN0 + 5) in call(amap, good, 0, 0, 64, outside)
    finally:
        plain.close()
        bare.close()
