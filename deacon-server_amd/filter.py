"""Host-side mirror of the reference's filter interface over the HIP C ABI.

Names, argument meaning and results follow the Rust items they stand for (paths under the reference's src/):

  Index                              <- index::load_minimizer_hashes            (index.rs:80-107)
  FilterProcessor                    <- local_filter::FilterProcessor          (local_filter.rs:153-285)
    .should_keep_sequence(seq)          (local_filter.rs:221-252)  -> (keep, hit_count, num_minimizers)
    .should_keep_pair(seq1, seq2)       (local_filter.rs:254-285)
    .filter_batch(...)                  the whole paraseq per-record loop   (local_filter.rs:346-528)
    .stats()                            ProcessingStats                        (local_filter.rs:179-187)
  get_minimizer_hashes_and_positions <- filter_common.rs:211-310
  IndexBuilder                       (no counterpart) an index built call by call that counts its keys' occurrences
  IndexSet / Classifier              (no counterpart) several indexes in one table, per-member hits in one pass
  Locator                            (no counterpart) where in each read an index or a set matched: segments
  DepthTracker                       (no counterpart) a set's depth counters binned along each sequence of a batch
  unpaired_should_keep / paired_should_keep <- remote_filter.rs:230-301

Everything here is plumbing: all arithmetic happens in lib/libdeacon_hip.so on the GPU.
"""
import ctypes as C
import os

import numpy as np

from . import _native as N
from ._native import DeaconHipError, Params

DEFAULT_KMER_LENGTH = 31  # minimizers.rs:4
DEFAULT_WINDOW_SIZE = 15  # minimizers.rs:5


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _as_u8(seq):
    if isinstance(seq, np.ndarray):
        return np.ascontiguousarray(seq, dtype=np.uint8)
    if isinstance(seq, str):
        seq = seq.encode()
    return np.frombuffer(bytes(seq), dtype=np.uint8)


def concat_reads(reads):
    """list of bytes-like -> (bases u8[], offsets u64[n+1]) in the layout dcn_filter_batch takes."""
    n = len(reads)
    offsets = np.zeros(n + 1, np.uint64)
    if n:
        np.cumsum(np.fromiter((len(r) for r in reads), dtype=np.uint64, count=n), out=offsets[1:])
    joined = b"".join(bytes(r) if not isinstance(r, str) else r.encode() for r in reads)
    bases = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(0, np.uint8)
    return bases, offsets


def _batch(bases, offsets):
    """a batch as the ABI takes it -> (bases u8[], offsets u64[n_reads+1], n_reads)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    return _as_u8(bases), offsets, len(offsets) - 1


class _Context:
    """Owner of one dcn_ctx, `_h`, over an index, a set or an anchor map: what Classifier, Locator, DepthTracker, Placer and
    FilterProcessor share, and what an AnchorMap holds for its adds."""

    def __init__(self, target_handle, max_batch_bases=1 << 26, max_batch_reads=1 << 20):
        self.max_batch_bases = int(max_batch_bases)
        self.max_batch_reads = int(max_batch_reads)
        self._h = C.c_void_p()
        N.check(N.lib().dcn_ctx_create(target_handle, self.max_batch_bases, self.max_batch_reads, C.byref(self._h)))

    def synchronize(self):
        N.check(N.lib().dcn_ctx_synchronize(self._h))

    @property
    def stream(self):
        return N.lib().dcn_ctx_stream(self._h)

    def stats(self):
        c = (C.c_uint64 * N.N_STATS)()
        N.check(N.lib().dcn_ctx_stats(self._h, c))
        return dict(zip(N.STAT_NAMES, (int(x) for x in c)))

    def set_profiling(self, enable=True):
        N.check(N.lib().dcn_ctx_set_profiling(self._h, 1 if enable else 0))

    def profile(self):
        """-> ({stage: accumulated device ms}, batches measured); HIP events on the context's stream.  What the 'distinct'
        and 'finish' slots hold depends on the call: see the class."""
        ms = (C.c_double * N.N_STAGES)()
        n = C.c_uint64()
        N.check(N.lib().dcn_ctx_profile(self._h, ms, C.byref(n)))
        return dict(zip(N.STAGE_NAMES, (float(x) for x in ms))), int(n.value)

    def close(self):
        if getattr(self, "_h", None):
            N.lib().dcn_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_ascii(bases, allow_newline=False):
    """Concatenated ASCII -> (packed u32[2*ceil(n/32)], invmask u32[ceil(n/32)]) in the layout
    dcn_filter_batch_packed takes (PackedSeqVec::from_ascii + the mask loop, filter_common.rs:238-258).
    A newline byte in the input raises: the ASCII entry points strip one from the end of a read
    (filter_common.rs:229), the packed ones cannot, so such a batch must go through filter_batch / submit."""
    bases = _as_u8(bases)
    g = (len(bases) + 31) // 32
    packed = np.zeros(max(2 * g, 1), np.uint32)
    mask = np.zeros(max(g, 1), np.uint32)
    nl = C.c_uint32()
    N.check(N.lib().dcn_pack_ascii(_ptr(bases) if len(bases) else None, len(bases), _ptr(packed), _ptr(mask), C.byref(nl)))
    if nl.value and not allow_newline:
        raise ValueError("pack_ascii: the batch holds a newline byte; a read ending in one is shortened by the ASCII entry "
                         "points (filter_common.rs:229) but not by the packed ones -- strip line ends or use filter_batch")
    return packed[:2 * g], mask[:g]


def set_minimizer_variant(nt_rot=1, cmp_bits=16, combine="add"):
    """Process-wide parity-pinning switch (include/deacon_hip.h): ntHash rotation per base, hash bits the window
    minimum compares, and how the strands' hashes are combined ("add" | "xor").  (1, 16, "add") are the rules of
    SURVEY.md 8a row A4; set it before any index is built or loaded."""
    N.check(N.lib().dcn_set_minimizer_variant(int(nt_rot), int(cmp_bits), {"add": 0, "xor": 1}[combine]))


def get_minimizer_variant():
    r, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    N.check(N.lib().dcn_get_minimizer_variant(C.byref(r), C.byref(b), C.byref(c)))
    return r.value, b.value, ("add", "xor")[c.value]


class PendingBatch:
    """A batch in flight (dcn_filter_batch_submit): holds the arrays the library reads and writes until wait()."""

    def __init__(self, proc, ticket, n_units, keep, hits, total, inputs):
        self.proc, self.ticket, self.n_units = proc, ticket, n_units
        self.keep, self.hits, self.total, self._inputs = keep, hits, total, inputs

    def wait(self):
        N.check(N.lib().dcn_filter_batch_wait(self.proc._h, self.ticket))
        self._inputs = None
        keep = self.keep[:self.n_units].astype(bool)
        if self.hits is None:
            return keep
        return keep, self.hits[:self.n_units], self.total[:self.n_units]


class PinnedBuffer:
    """Page-locked host memory from dcn_host_alloc, viewed as a numpy array: batches built in one go over PCIe
    without the staging copy.  Keep the object alive while `.array` is in use."""

    def __init__(self, count, dtype=np.uint8):
        dtype = np.dtype(dtype)
        self._p = C.c_void_p()
        self.nbytes = int(count) * dtype.itemsize
        N.check(N.lib().dcn_host_alloc(self.nbytes, C.byref(self._p)))
        raw = (C.c_uint8 * max(self.nbytes, 1)).from_address(self._p.value)
        self.array = np.frombuffer(raw, dtype=dtype, count=int(count))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.array = None
            N.lib().dcn_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index:
    """Device-resident minimizer set (stands for Arc<FxHashSet<u64>> + IndexHeader)."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device
        k, w, n = C.c_uint8(), C.c_uint8(), C.c_uint64()
        N.check(N.lib().dcn_index_header(self._h, C.byref(k), C.byref(w), C.byref(n)))
        self.kmer_length, self.window_size, self.n_keys = k.value, w.value, n.value

    @classmethod
    def from_keys(cls, keys, kmer_length=DEFAULT_KMER_LENGTH, window_size=DEFAULT_WINDOW_SIZE, device=0):
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
        h = C.c_void_p()
        N.check(N.lib().dcn_index_from_keys(_ptr(keys), len(keys), kmer_length, window_size, device, C.byref(h)))
        return cls(h, device)

    @classmethod
    def from_file(cls, path, device=0):
        h = C.c_void_p()
        N.check(N.lib().dcn_index_from_file(os.fsencode(path), device, C.byref(h)))
        return cls(h, device)

    @classmethod
    def build(cls, seqs, kmer_length=DEFAULT_KMER_LENGTH, window_size=DEFAULT_WINDOW_SIZE, entropy_threshold=0.0,
              capacity_keys=0, device=0):
        """index::build (index.rs:167-308) for sequences in memory: index-side minimizers merged on the device."""
        bases, offsets = concat_reads(seqs)
        h = C.c_void_p()
        N.check(N.lib().dcn_index_build(_ptr(bases) if len(bases) else None, _ptr(offsets), len(seqs), kmer_length,
                                        window_size, float(entropy_threshold), int(capacity_keys), device, C.byref(h)))
        return cls(h, device)

    @classmethod
    def union(cls, indexes):
        """index::union (index.rs:563-664): set union; all inputs must share k and w."""
        arr = (C.c_void_p * len(indexes))(*[i._h for i in indexes])
        h = C.c_void_p()
        N.check(N.lib().dcn_index_union(arr, len(indexes), C.byref(h)))
        return cls(h, indexes[0].device)

    @classmethod
    def intersect(cls, indexes):
        """The minimizers present in every one of `indexes` (dcn_index_intersect; no reference counterpart): same k, w,
        minimizer rule and device, any number of them; the result is sized for its own key count."""
        indexes = list(indexes)
        arr = (C.c_void_p * max(len(indexes), 1))(*[i._h for i in indexes])
        h = C.c_void_p()
        N.check(N.lib().dcn_index_intersect(arr, len(indexes), C.byref(h)))
        return cls(h, indexes[0].device)

    def clone(self, device):
        """Replica on another (or the same) device, copied device to device (dcn_index_clone)."""
        h = C.c_void_p()
        N.check(N.lib().dcn_index_clone(self._h, int(device), C.byref(h)))
        return type(self)(h, int(device))

    @property
    def table_bytes(self):
        """device memory of the hash table (dcn_index_memory)"""
        b = C.c_uint64()
        N.check(N.lib().dcn_index_memory(self._h, C.byref(b)))
        return b.value

    def diff(self, other):
        """index::diff (index.rs:421-536): the minimizers of self that are not in other."""
        h = C.c_void_p()
        N.check(N.lib().dcn_index_diff(self._h, other._h, C.byref(h)))
        return type(self)(h, self.device)

    def keys(self):
        """The distinct minimizer hashes (arbitrary order, like iterating the reference's set)."""
        out = np.zeros(max(self.n_keys, 1), np.uint64)
        n = C.c_uint64()
        N.check(N.lib().dcn_index_keys(self._h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    def write(self, path):
        """index::write_minimizers (index.rs:130-164): the reference's index file format."""
        N.check(N.lib().dcn_index_write_file(self._h, os.fsencode(path)))

    def header(self):
        return self.kmer_length, self.window_size, self.n_keys

    def __len__(self):
        return self.n_keys

    def contains(self, keys):
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
        out = np.zeros(len(keys), np.uint8)
        N.check(N.lib().dcn_index_contains(self._h, _ptr(keys), len(keys), _ptr(out)))
        return out.astype(bool)

    def contains_device(self, d_keys, n, d_out, stream=None):
        """Device-resident probe: d_keys / d_out are raw device pointers; asynchronous on `stream`."""
        N.check(N.lib().dcn_index_contains_device(self._h, d_keys, n, d_out, stream))

    def probe_ceiling(self, d_keys=None, n=64_000_000, reps=5):
        """Home-group reads per second this table serves for a key stream (device pointer; None: uniformly random
        groups) with nothing else running -- dcn_index_probe_ceiling."""
        r = C.c_double()
        N.check(N.lib().dcn_index_probe_ceiling(self._h, d_keys, n, reps, C.byref(r)))
        return r.value

    def close(self):
        if getattr(self, "_h", None):
            N.lib().dcn_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IndexBuilder:
    """An index built over several calls that counts how often each key occurs (dcn_index_builder_*; no reference
    counterpart).  add() takes sequences batch by batch -- the index-side rule of Index.build, an occurrence being a distinct
    (sequence, position) pair -- and finish() hands out plain indexes by count: min_count for indexes built from reads,
    max_count for repeat-aware ones.  Counts are 16 bits and saturate at 65,535.  Not thread-safe."""

    def __init__(self, kmer_length=DEFAULT_KMER_LENGTH, window_size=DEFAULT_WINDOW_SIZE, entropy_threshold=0.0,
                 capacity_keys=0, device=0):
        for name, v, hi in (("kmer_length", kmer_length, 255), ("window_size", window_size, 255),
                            ("capacity_keys", capacity_keys, (1 << 64) - 1)):
            if not 0 <= int(v) <= hi:
                raise ValueError(f"{name} {v} out of range")
        self._h = C.c_void_p()
        self.device = int(device)
        self.kmer_length, self.window_size = int(kmer_length), int(window_size)
        N.check(N.lib().dcn_index_builder_create(int(kmer_length), int(window_size), float(entropy_threshold),
                                                 int(capacity_keys), int(device), C.byref(self._h)))

    def add(self, seqs):
        """count and insert the index-side minimizers of every sequence of `seqs` (bytes-like each)"""
        seqs = list(seqs)
        bases, offsets = concat_reads(seqs)
        N.check(N.lib().dcn_index_builder_add(self._h, _ptr(bases) if len(bases) else None, _ptr(offsets), len(seqs)))

    def info(self):
        """{"n_keys", "n_occurrences" (the true number, not the saturated sum), "n_bases", "device_bytes"}"""
        v = [C.c_uint64() for _ in range(4)]
        N.check(N.lib().dcn_index_builder_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_keys", "n_occurrences", "n_bases", "device_bytes"), (x.value for x in v)))

    def __len__(self):
        return self.info()["n_keys"]

    def hist(self, n_bins=256):
        """np.uint64[n_bins]: keys by count, the last bin holding every count >= n_bins - 1; bin 0 is always 0"""
        if not 0 <= int(n_bins) <= 0xFFFFFFFF:
            raise ValueError(f"n_bins {n_bins} out of range")
        hist = np.zeros(max(int(n_bins), 1), np.uint64)
        N.check(N.lib().dcn_index_builder_hist(self._h, int(n_bins), _ptr(hist)))
        return hist

    def counts(self):
        """(keys np.uint64, counts np.uint32) of every key, in no particular order"""
        n = C.c_uint64()
        rc = N.lib().dcn_index_builder_counts(self._h, None, None, 0, C.byref(n))
        if rc != N.DCN_ERR_CAPACITY:
            N.check(rc)
        keys = np.zeros(max(n.value, 1), np.uint64)
        counts = np.zeros(max(n.value, 1), np.uint32)
        N.check(N.lib().dcn_index_builder_counts(self._h, _ptr(keys), _ptr(counts), len(keys), C.byref(n)))
        return keys[:n.value], counts[:n.value]

    def finish(self, min_count=1, max_count=0, count_only=False):
        """The keys with min_count <= count <= max_count (0 = no upper bound): a new plain Index sized for them, or their
        number with count_only.  The builder stays as it is: finish again with other bounds, or add more."""
        for name, v in (("min_count", min_count), ("max_count", max_count)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} {v} out of range")
        n = C.c_uint64()
        h = C.c_void_p()
        N.check(N.lib().dcn_index_builder_finish(self._h, int(min_count), int(max_count), C.byref(n),
                                                 None if count_only else C.byref(h)))
        return n.value if count_only else Index(h, self.device)

    def close(self):
        if getattr(self, "_h", None):
            N.lib().dcn_index_builder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IndexSet:
    """Labelled index set (dcn_index_set_create): one device table over the union of 1..32 indexes of equal k, w,
    minimizer rule and device, each key carrying a mask of the members that hold it (bit j = indexes[j]).  The set owns
    its memory: the member Index objects may be closed afterwards."""

    def __init__(self, indexes):
        indexes = list(indexes)
        arr = (C.c_void_p * max(len(indexes), 1))(*[i._h for i in indexes])
        self._h = C.c_void_p()
        N.check(N.lib().dcn_index_set_create(arr, len(indexes), C.byref(self._h)))
        self.device = indexes[0].device
        n, k, w = C.c_uint32(), C.c_uint8(), C.c_uint8()
        keys, mem = C.c_uint64(), C.c_uint64()
        N.check(N.lib().dcn_index_set_info(self._h, C.byref(n), C.byref(k), C.byref(w), C.byref(keys), C.byref(mem)))
        self.n, self.k, self.w, self.n_keys, self.memory = n.value, k.value, w.value, keys.value, mem.value

    # ---- coverage (dcn_index_set_coverage*): distinct keys of each member observed by classify calls on this set ----
    def enable_coverage(self, on=True):
        """Allocate a zeroed observed-bitmap (on) or free it (off); every later classify call against the set, from
        any Classifier, marks the set's keys among its units' counted minimizers.  Enabling twice keeps the marks."""
        N.check(N.lib().dcn_index_set_coverage_enable(self._h, 1 if on else 0))

    def reset_coverage(self):
        N.check(N.lib().dcn_index_set_coverage_reset(self._h))

    def coverage(self):
        """(observed, keys): np.uint64[n] each -- keys[j] distinct keys of member j in the set, observed[j] how many of
        them were marked.  Device-form batches must have been synchronized first."""
        observed = np.zeros(self.n, np.uint64)
        keys = np.zeros(self.n, np.uint64)
        N.check(N.lib().dcn_index_set_coverage(self._h, _ptr(observed), _ptr(keys)))
        return observed, keys

    def observed_keys(self, member=None):
        """the observed keys of member `member` (None: of any member), np.uint64 in no particular order"""
        m = 0xFFFFFFFF if member is None else int(member)
        if not 0 <= m <= 0xFFFFFFFF:
            raise ValueError(f"member {member} out of range")
        n = C.c_uint64()
        rc = N.lib().dcn_index_set_coverage_keys(self._h, m, None, 0, C.byref(n))
        if rc != N.DCN_ERR_CAPACITY:
            N.check(rc)
        out = np.zeros(max(n.value, 1), np.uint64)
        N.check(N.lib().dcn_index_set_coverage_keys(self._h, m, _ptr(out), len(out), C.byref(n)))
        return out[:n.value]

    # ---- depth (dcn_index_set_depth_*): how often each key occurred among the minimizers classify calls counted ----
    def enable_depth(self, on=True):
        """Allocate zeroed 16-bit counters, one per slot (on), or free them (off); every later classify call against the
        set, from any Classifier, adds its occurrences (saturating at 65,535).  Enabling twice keeps the counts."""
        N.check(N.lib().dcn_index_set_depth_enable(self._h, 1 if on else 0))

    def reset_depth(self):
        N.check(N.lib().dcn_index_set_depth_reset(self._h))

    def depth_stats(self):
        """{"observed", "sum", "saturated"}: np.uint64[n] each, over member j's keys -- keys with depth > 0, the sum of
        their depths, keys at 65,535.  Device-form batches must have been synchronized first."""
        out = {name: np.zeros(self.n, np.uint64) for name in ("observed", "sum", "saturated")}
        N.check(N.lib().dcn_index_set_depth_stats(self._h, _ptr(out["observed"]), _ptr(out["sum"]), _ptr(out["saturated"])))
        return out

    def depth_hist(self, member=None, n_bins=256):
        """np.uint64[n_bins]: keys of member `member` (None: of any member) by depth, the last bin holding every depth
        >= n_bins - 1 and bin 0 the unobserved keys"""
        m = 0xFFFFFFFF if member is None else int(member)
        if not 0 <= m <= 0xFFFFFFFF or not 0 <= int(n_bins) <= 0xFFFFFFFF:
            raise ValueError(f"member {member} / n_bins {n_bins} out of range")
        hist = np.zeros(max(int(n_bins), 1), np.uint64)
        N.check(N.lib().dcn_index_set_depth_hist(self._h, m, int(n_bins), _ptr(hist)))
        return hist

    def depth_keys(self, member=None):
        """(keys np.uint64, depths np.uint32) of the keys of member `member` (None: of any member) with depth > 0, in no
        particular order"""
        m = 0xFFFFFFFF if member is None else int(member)
        if not 0 <= m <= 0xFFFFFFFF:
            raise ValueError(f"member {member} out of range")
        n = C.c_uint64()
        rc = N.lib().dcn_index_set_depth_keys(self._h, m, None, None, 0, C.byref(n))
        if rc != N.DCN_ERR_CAPACITY:
            N.check(rc)
        keys = np.zeros(max(n.value, 1), np.uint64)
        depths = np.zeros(max(n.value, 1), np.uint32)
        N.check(N.lib().dcn_index_set_depth_keys(self._h, m, _ptr(keys), _ptr(depths), len(keys), C.byref(n)))
        return keys[:n.value], depths[:n.value]

    # ---- set algebra on the member masks (dcn_index_set_select / dcn_index_set_overlap) ----
    def __len__(self):
        return self.n_keys

    def _mask(self, members):
        """a member mask given as an int, or as an iterable of member numbers"""
        if isinstance(members, (int, np.integer)):
            m = int(members)
        else:
            m = 0
            for j in members:
                if not 0 <= int(j) < 32:
                    raise ValueError(f"member {j} out of range")
                m |= 1 << int(j)
        if not 0 <= m <= 0xFFFFFFFF:
            raise ValueError(f"member mask {members} out of range")
        return m

    def select(self, all_of=0, any_of=0, none_of=0, min_members=0, max_members=0, count_only=False):
        """The keys whose member mask L holds every member of all_of, some member of any_of (if given), none of none_of,
        and min_members <= popcount(L) <= max_members (0 = no bound): a new plain Index sized for them, or their number
        with count_only.  Masks are ints (bit j = member j) or iterables of member numbers.  The member-specific keys of
        member j: select(all_of=[j], max_members=1); the core held by at least m members: select(min_members=m)."""
        n = C.c_uint64()
        h = C.c_void_p()
        N.check(N.lib().dcn_index_set_select(self._h, self._mask(all_of), self._mask(any_of), self._mask(none_of),
                                             int(min_members), int(max_members), C.byref(n),
                                             None if count_only else C.byref(h)))
        return n.value if count_only else Index(h, self.device)

    def overlap(self):
        """How much the members share: {"shared": u64[n, n] (keys in members i and j; the diagonal is each member's key
        count), "exclusive": u64[n] (keys in member j alone), "by_count": u64[n] (keys held by exactly c + 1 members)}."""
        shared = np.zeros((self.n, self.n), np.uint64)
        exclusive = np.zeros(self.n, np.uint64)
        by_count = np.zeros(self.n, np.uint64)
        N.check(N.lib().dcn_index_set_overlap(self._h, _ptr(shared), _ptr(exclusive), _ptr(by_count)))
        return {"shared": shared, "exclusive": exclusive, "by_count": by_count}

    def close(self):
        if getattr(self, "_h", None):
            N.lib().dcn_index_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Classifier(_Context):
    """Per-member classification of batches against an IndexSet (dcn_classify_batch): for every unit (read, or pair
    through unit_id) the distinct hits against each member, the minimizer count, and a bit mask of the members whose
    thresholds the unit meets (the search-mode decision of FilterProcessor against that member alone).
    profile(): for classify calls the stages are pack, plan, scan (minimizer dump), and the two classification kernels in
    the 'distinct' (one lane per unit) and 'finish' (one workgroup per large unit) slots."""

    def __init__(self, index_set, abs_threshold=2, rel_threshold=0.01, prefix_length=0, device=None,
                 max_batch_bases=1 << 26, max_batch_reads=1 << 20):
        if device is not None and int(device) != index_set.device:
            raise ValueError(f"the set lives on device {index_set.device}, not {device}")
        self.index_set = index_set
        self.abs_threshold = int(abs_threshold)
        self.rel_threshold = float(rel_threshold)
        self.prefix_length = int(prefix_length)
        super().__init__(index_set._h, max_batch_bases, max_batch_reads)

    def _params(self):
        return Params(self.abs_threshold, self.rel_threshold, self.prefix_length, 0, 0)

    def classify_batch(self, bases, offsets, unit_id=None):
        """bases: concatenated ASCII; offsets[n_reads+1]; unit_id groups mates ->
        (match u32[n_units], hits u32[n_units, n], total u32[n_units])"""
        bases, offsets, n_reads = _batch(bases, offsets)
        if unit_id is not None:
            unit_id = np.ascontiguousarray(unit_id, dtype=np.uint32)
            n_units = int(unit_id[-1]) + 1 if n_reads else 0
        else:
            n_units = n_reads
        n = self.index_set.n
        match = np.zeros(max(n_units, 1), np.uint32)
        hits = np.zeros((max(n_units, 1), n), np.uint32)
        total = np.zeros(max(n_units, 1), np.uint32)
        p = self._params()
        N.check(N.lib().dcn_classify_batch(self._h, self.index_set._h, _ptr(bases) if len(bases) else None,
                                           _ptr(offsets), _ptr(unit_id), n_reads, C.byref(p), _ptr(match), _ptr(hits),
                                           _ptr(total)))
        return match[:n_units], hits[:n_units], total[:n_units]

    def classify_batch_device(self, d_bases, d_offsets, n_reads, n_bases, d_match, d_hits=None, d_total=None,
                              d_unit_id=None, n_units=None):
        """Same on device-resident inputs (raw device pointers); asynchronous: synchronize() before reading."""
        p = self._params()
        if n_units is None:
            n_units = n_reads
        N.check(N.lib().dcn_classify_batch_device(self._h, self.index_set._h, d_bases, d_offsets, d_unit_id, n_reads,
                                                  n_bases, n_units, C.byref(p), d_match, d_hits, d_total))


# numpy view of dcn_segment (16 bytes)
SEGMENT_DTYPE = np.dtype([("start", np.uint32), ("end", np.uint32), ("n_hits", np.uint32), ("members", np.uint32)])


class Locator(_Context):
    """Where in each read an Index or an IndexSet matched (dcn_locate_batch; the definition of a segment is in
    include/deacon_hip.h): per read, the half-open [start, end) stretches its hit minimizer k-mers cover once hits at most
    max_gap bases apart are joined, with the number of hit positions and the OR of their member labels.
    max_gap=None is the derived default 2*w - 1; member_mask selects members of a set (ignored for a plain index).
    profile(): pack, plan, scan (minimizer dump), the probe sweep that marks hits in the 'distinct' slot and the segment
    passes (count, scan over reads, write) in the 'finish' slot."""

    def __init__(self, index, max_gap=None, min_hits=1, prefix_length=0, member_mask=0xFFFFFFFF,
                 max_batch_bases=1 << 26, max_batch_reads=1 << 20):
        self.index = index
        w = index.w if hasattr(index, "w") else index.window_size  # (IndexSet / Index)
        self.max_gap = 2 * int(w) - 1 if max_gap is None else int(max_gap)
        self.min_hits = int(min_hits)
        self.prefix_length = int(prefix_length)
        self.member_mask = int(member_mask)
        super().__init__(index._h, max_batch_bases, max_batch_reads)

    def _params(self):
        return N.LocateParams(self.max_gap, self.min_hits, self.member_mask, 0, self.prefix_length)

    def locate_batch(self, bases, offsets):
        """bases: concatenated ASCII; offsets[n_reads+1] -> (seg_offsets u64[n_reads+1], segs SEGMENT_DTYPE[]): read r
        owns segs[seg_offsets[r]:seg_offsets[r+1]], ascending by start."""
        bases, offsets, n_reads = _batch(bases, offsets)
        seg_offsets = np.zeros(n_reads + 1, np.uint64)
        p = self._params()
        cap = getattr(self, "_last_total", 0)
        segs = np.zeros(max(cap, 1), SEGMENT_DTYPE)
        for _ in range(2):  # the second call has the capacity the first one asked for
            rc = N.lib().dcn_locate_batch(self._h, self.index._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                          n_reads, C.byref(p), _ptr(seg_offsets), _ptr(segs) if cap else None, cap)
            if rc != N.DCN_ERR_CAPACITY:
                break
            cap = int(seg_offsets[n_reads])
            segs = np.zeros(cap, SEGMENT_DTYPE)
        N.check(rc)
        self._last_total = int(seg_offsets[n_reads])
        return seg_offsets, segs[:int(seg_offsets[n_reads])]


# numpy view of dcn_track_bin (24 bytes)
TRACK_BIN_DTYPE = np.dtype([("n_positions", np.uint32), ("n_keys", np.uint32), ("n_observed", np.uint32),
                            ("max_depth", np.uint32), ("sum_depth", np.uint64)])


class DepthTracker(_Context):
    """Depth tracks (dcn_depth_track_batch; the definition of a bin is in include/deacon_hip.h): for every sequence of a
    batch, bins of bin_bases bases (0: one bin per sequence), each with the number of minimizer positions that start in
    it, how many of them are keys of the chosen members, how many of those the classify calls on the set have seen, and
    the sum and the maximum of their depth counters (each capped at depth_cap when that is not 0).  The set has depth
    enabled; its counters are read, never changed.  member=None: every member; an int or an iterable selects members.
    profile(): pack, plan, scan (minimizer dump), the probe sweep that marks positions and reads the counters in the
    'distinct' slot and the reduction into bins in the 'finish' slot."""

    def __init__(self, index_set, max_batch_bases=1 << 26, max_batch_reads=1 << 20, bin_bases=1000, member=None,
                 depth_cap=0, prefix_length=0):
        self.index_set = index_set
        self.bin_bases = int(bin_bases)
        if member is None:
            self.member_mask = (1 << index_set.n) - 1
        elif isinstance(member, (int, np.integer)):
            if int(member) < 0:
                raise ValueError(f"member {member} out of range")
            self.member_mask = 1 << int(member)
        else:
            self.member_mask = index_set._mask(member)
        self.depth_cap = int(depth_cap)
        self.prefix_length = int(prefix_length)
        if not (0 <= self.bin_bases <= 0xFFFFFFFF and 0 <= self.member_mask <= 0xFFFFFFFF and 0 <= self.depth_cap <= 0xFFFFFFFF):
            raise ValueError("bin_bases / member / depth_cap out of range")
        super().__init__(index_set._h, max_batch_bases, max_batch_reads)

    def _params(self):
        return N.TrackParams(self.bin_bases, self.member_mask, self.depth_cap, 0, self.prefix_length)

    def track_batch(self, bases, offsets):
        """bases: concatenated ASCII; offsets[n_reads+1] -> (bin_offsets u64[n_reads+1], bins TRACK_BIN_DTYPE[]): read r
        owns bins[bin_offsets[r]:bin_offsets[r+1]], bin b of it covers its bases [b * bin_bases, (b + 1) * bin_bases)."""
        bases, offsets, n_reads = _batch(bases, offsets)
        bin_offsets = np.zeros(n_reads + 1, np.uint64)
        p = self._params()
        rc = N.lib().dcn_depth_track_batch(self._h, self.index_set._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                           n_reads, C.byref(p), _ptr(bin_offsets), None, 0)  # the count: no device work
        if rc != N.DCN_ERR_CAPACITY:
            N.check(rc)
            return bin_offsets, np.zeros(0, TRACK_BIN_DTYPE)
        total = int(bin_offsets[n_reads])
        bins = np.zeros(total, TRACK_BIN_DTYPE)
        N.check(N.lib().dcn_depth_track_batch(self._h, self.index_set._h, _ptr(bases) if len(bases) else None,
                                              _ptr(offsets), n_reads, C.byref(p), _ptr(bin_offsets), _ptr(bins), total))
        return bin_offsets, bins

    def track(self, seqs):
        """the tracks of a list of sequences: one TRACK_BIN_DTYPE array per sequence"""
        seqs = list(seqs)
        bases, offsets = concat_reads(seqs)
        bo, bins = self.track_batch(bases, offsets)
        return [bins[int(bo[r]):int(bo[r + 1])] for r in range(len(seqs))]


# numpy view of dcn_placement (48 bytes)
PLACEMENT_DTYPE = np.dtype([("record", np.uint32), ("reverse", np.uint32), ("votes", np.uint32), ("n_anchors", np.uint32),
                            ("n_positions", np.uint32), ("read_start", np.uint32), ("read_end", np.uint32),
                            ("reserved", np.uint32), ("ref_start", np.uint64), ("ref_end", np.uint64)])
UNPLACED = 0xFFFFFFFF
# numpy view of dcn_split_placement (64 bytes): the fields of dcn_placement, then rank, n_placed, rival_votes, mapq
SPLIT_PLACEMENT_DTYPE = np.dtype(PLACEMENT_DTYPE.descr + [("rank", np.uint32), ("n_placed", np.uint32),
                                                          ("rival_votes", np.uint32), ("mapq", np.uint32)])
# numpy view of dcn_pair_placement (80 bytes): the fields of dcn_split_placement, then flags, pair_votes, tlen
PAIR_PLACEMENT_DTYPE = np.dtype(SPLIT_PLACEMENT_DTYPE.descr + [("flags", np.uint32), ("pair_votes", np.uint32),
                                                               ("tlen", np.int64)])
PAIR_PROPER, PAIR_RESCUED, PAIR_MATE_PLACED = 1, 2, 4  # DCN_PAIR_*: bits of `flags`
# numpy view of dcn_extension (32 bytes): the four coordinates of an extended row and the edits of its two flanks
EXTENSION_DTYPE = np.dtype([("read_start", np.uint32), ("read_end", np.uint32), ("ref_start", np.uint64), ("ref_end", np.uint64),
                            ("left_edits", np.uint32), ("right_edits", np.uint32)])
VERIFY_OVER, VERIFY_UNPLACED = N.VERIFY_OVER, N.VERIFY_UNPLACED  # DCN_VERIFY_*: what `edits` holds instead of a distance
# DCN_PILEUP_*: the columns of AnchorMap.pileup_fetch, the flags of a site's info and the code of no call
PILEUP_A, PILEUP_C, PILEUP_G, PILEUP_T, PILEUP_N, PILEUP_DEL, PILEUP_INS, PILEUP_REV = (
    N.PILEUP_A, N.PILEUP_C, N.PILEUP_G, N.PILEUP_T, N.PILEUP_N, N.PILEUP_DEL, N.PILEUP_INS, N.PILEUP_REV)
PILEUP_COLUMNS = N.PILEUP_COLUMNS
PILEUP_SITE_SUB, PILEUP_SITE_DEL, PILEUP_SITE_INS, PILEUP_NO_CODE = N.PILEUP_SITE_SUB, N.PILEUP_SITE_DEL, N.PILEUP_SITE_INS, N.PILEUP_NO_CODE
# numpy views of dcn_insertion (24 bytes) and dcn_insertion_allele (32 bytes): an event of an insertion ledger and the
# called insertion of a position; bases_offset points into the bases returned beside them
INSERTION_DTYPE = np.dtype([("pos", np.uint64), ("bases_offset", np.uint64), ("len", np.uint32), ("flags", np.uint32)])
INSERTION_ALLELE_DTYPE = np.dtype([("pos", np.uint64), ("bases_offset", np.uint64), ("len", np.uint32), ("count", np.uint32),
                                   ("events", np.uint32), ("flags", np.uint32)])
INSERTION_FRONT, INSERTION_REVERSE = N.INSERTION_FRONT, N.INSERTION_REVERSE  # DCN_INSERTION_*: bits of `flags`
# dcn_genotype_site, 48 bytes: what AnchorMap.genotype returns per site
GENOTYPE_SITE_DTYPE = np.dtype([("pos", np.uint64), ("qual", np.uint32), ("depth", np.uint32), ("ad", np.uint32, (4,)), ("gt", np.uint8),
                                ("gq", np.uint8), ("ref_code", np.uint8), ("reserved0", np.uint8), ("pl", np.uint8, (10,)),
                                ("reserved1", np.uint8, (2,))])
GENOTYPE_NONE, GENOTYPES = N.GENOTYPE_NONE, N.GENOTYPES
# numpy views of dcn_deletion (16 bytes) and dcn_indel_site (48 bytes): an event of a deletion ledger, and what
# AnchorMap.indels_genotype returns per site; bases_offset points into the bases returned beside the sites
DELETION_DTYPE = np.dtype([("pos", np.uint64), ("len", np.uint32), ("flags", np.uint32)])
# dcn_left_align_info: the rows with an alignment, and of those the rows in which a gap took a step, the gaps that took one, their steps
# and the times two gaps became one
LEFT_ALIGN_INFO_DTYPE = np.dtype([("rows_aligned", np.uint64), ("rows_changed", np.uint64), ("gaps_shifted", np.uint64),
                                  ("columns_passed", np.uint64), ("gaps_merged", np.uint64)])
INDEL_SITE_DTYPE = np.dtype([("pos", np.uint64), ("bases_offset", np.uint64), ("len", np.uint32), ("flags", np.uint32), ("qual", np.uint32),
                             ("depth", np.uint32), ("count", np.uint32), ("events", np.uint32), ("gt", np.uint8), ("gq", np.uint8),
                             ("pl", np.uint8, (3,)), ("reserved", np.uint8, (3,))])
DELETION_REVERSE, INDEL_DELETION, INDEL_FRONT = N.DELETION_REVERSE, N.INDEL_DELETION, N.INDEL_FRONT  # DCN_DELETION_*, DCN_INDEL_*
# numpy views of dcn_strand_query (32 bytes) and dcn_strand_site (64 bytes): what AnchorMap.strand_evidence takes and returns
STRAND_QUERY_DTYPE = np.dtype([("pos", np.uint64), ("kind", np.uint32), ("ref_code", np.uint32), ("alt_mask", np.uint32), ("count", np.uint32),
                               ("count_reverse", np.uint32), ("reserved", np.uint32)])
STRAND_SITE_DTYPE = np.dtype([("fwd", np.uint32, (4,)), ("rev", np.uint32, (4,)), ("table", np.uint32, (4,)), ("sb_centi", np.uint32),
                              ("flags", np.uint32), ("reserved", np.uint32, (2,))])
STRAND_BIAS, STRAND_ONE_SIDED = N.STRAND_BIAS, N.STRAND_ONE_SIDED  # DCN_STRAND_*
# dcn_reference_block (include/deacon_hip_blocks.h), 40 bytes: what AnchorMap.reference_blocks returns per block
REFERENCE_BLOCK_DTYPE = np.dtype([("pos", np.uint64), ("sum_depth", np.uint64), ("len", np.uint32), ("min_depth", np.uint32),
                                  ("max_depth", np.uint32), ("min_gq", np.uint32), ("cls", np.uint32), ("reserved", np.uint32)])
BLOCK_NO_COVERAGE, BLOCK_UNCALLED, BLOCK_REF, BLOCK_VARIANT = N.BLOCK_NO_COVERAGE, N.BLOCK_UNCALLED, N.BLOCK_REF, N.BLOCK_VARIANT  # DCN_BLOCK_*
# dcn_phase_site (16 bytes) and dcn_phase_result (32 bytes) of include/deacon_hip_phase.h: what AnchorMap.phase_sites takes and
# AnchorMap.phase_solve returns per site
PHASE_SITE_DTYPE = np.dtype([("pos", np.uint64), ("record", np.uint32), ("a0", np.uint8), ("a1", np.uint8), ("reserved", np.uint8, (2,))])
PHASE_RESULT_DTYPE = np.dtype([("set_pos", np.uint64), ("link", np.uint32, (4,)), ("set_index", np.uint32), ("hap", np.uint8),
                               ("flags", np.uint8), ("reserved", np.uint8, (2,))])
PHASE_HEAD, PHASE_JOINED = N.PHASE_HEAD, N.PHASE_JOINED  # DCN_PHASE_*
_CIGAR_LETTERS = {N.CIGAR_INS: "I", N.CIGAR_DEL: "D", N.CIGAR_EQUAL: "=", N.CIGAR_DIFF: "X"}


def cigar_string(ops):
    """the runs of one row of Placer.align_batch (len << 4 | op, BAM's codes) -> "12=1X3I..." ("" for no runs)"""
    return "".join("%d%s" % (int(x) >> 4, _CIGAR_LETTERS[int(x) & 15]) for x in ops)


class AnchorMap(Index):
    """An index whose slots know where on a reference their key lies (dcn_anchor_map_*; the definition of an anchor is in
    include/deacon_hip.h): a copy of `index`'s keys (the source may be closed afterwards) with one word per slot.  Records
    are numbered in the order they are added; a key that occurs at exactly one (record, position) of them is an anchor, one
    that occurs at several is a repeat and never votes.  It is an Index: contexts can be created over it, clone() gives a
    plain Index without the words.  keep_bases=True also keeps the bases of every record on the device (0.375 B per base;
    dcn_anchor_map_keep_bases): fetch() cuts a region out, and Placer.verify_batch compares placements base by base."""

    def __init__(self, index, keep_bases=False):
        h = C.c_void_p()
        N.check(N.lib().dcn_anchor_map_create(index._h, C.byref(h)))
        super().__init__(h, index.device)
        self._ctx = None
        self.keeps_bases = bool(keep_bases)
        self._record_lengths = []
        if keep_bases:
            N.check(N.lib().dcn_anchor_map_keep_bases(self._h))

    def fetch(self, record, start, n):
        """bases [start, start + n) of a record -> bytes: ACGT, and N for every base that was not in ACGTacgt"""
        out = np.zeros(max(int(n), 1), np.uint8)
        N.check(N.lib().dcn_anchor_map_fetch(self._h, int(record), int(start), int(n), _ptr(out)))
        return out[:int(n)].tobytes()

    def pileup_enable(self):
        """Eight uint32 counters per base of the records added so far, all zero (dcn_anchor_map_pileup_enable; the
        definition of a pileup is in include/deacon_hip.h): 32 B of device memory per kept base.  The map must keep
        bases; while the pileup is enabled add() is refused.  Placer.pileup_batch adds rows to it."""
        N.check(N.lib().dcn_anchor_map_pileup_enable(self._h, 1))

    def pileup_disable(self):
        N.check(N.lib().dcn_anchor_map_pileup_enable(self._h, 0))

    def pileup_reset(self):
        """every counter back to zero"""
        N.check(N.lib().dcn_anchor_map_pileup_reset(self._h))

    def pileup_fetch(self, record, start=0, n=None):
        """the counters of positions [start, start + n) of a record (n=None: to its end) -> np.uint32[n, 8], the columns
        PILEUP_A, C, G, T, N, DEL, INS, REV"""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        out = np.zeros((max(n, 1), N.PILEUP_COLUMNS), np.uint32)
        N.check(N.lib().dcn_anchor_map_pileup_fetch(self._h, int(record), start, n, _ptr(out)))
        return out[:n]

    def pileup_call(self, record, start=0, n=None, min_depth=3, min_permille=500):
        """Rule P6 over positions [start, start + n) of a record (n=None: to its end) -> (calls bytes of ACGT-N, site_pos
        np.uint64[], site_info np.uint32[]): the sites in ascending record position, info = flags (PILEUP_SITE_SUB / _DEL /
        _INS) | call_code << 8 | ref_code << 16.  min_depth = 3 and min_permille = 500 are conventions, not measured
        optima.  One call with an estimate and, on DCN_ERR_CAPACITY, a second with the size the first reported."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        p = N.PileupCallParams(int(min_depth), int(min_permille), (C.c_uint32 * 2)(0, 0))
        calls = np.zeros(max(n, 1), np.uint8)
        n_sites = C.c_uint64()

        def call(cap):
            pos, info = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32)
            rc = N.lib().dcn_anchor_map_pileup_call(self._h, C.byref(p), int(record), start, n, _ptr(calls), _ptr(pos) if cap else None,
                                                    _ptr(info) if cap else None, cap, C.byref(n_sites))
            return rc, pos, info

        rc, pos, info = call(n // 64 + 64)
        if rc == N.DCN_ERR_CAPACITY:
            rc, pos, info = call(int(n_sites.value))
        N.check(rc)
        return calls[:n].tobytes(), pos[:int(n_sites.value)], info[:int(n_sites.value)]

    def pileup_keep_insertions(self, keep=True):
        """An insertion ledger beside the pileup (dcn_anchor_map_pileup_keep_insertions; the definition of an insertion
        ledger is in include/deacon_hip.h): every I run that Placer.pileup_batch counts in INS also leaves its bases.
        Refused once a row has added since pileup_enable() or pileup_reset(); keep=False drops it and leaves the counters."""
        N.check(N.lib().dcn_anchor_map_pileup_keep_insertions(self._h, 1 if keep else 0))

    def pileup_keep_qualities(self, keep=True):
        """Quality sums beside the pileup (dcn_anchor_map_pileup_keep_qualities; the definition of a quality-aware pileup is
        in include/deacon_hip.h): four uint32 per base, to which Placer.pileup_batch(..., quals=) adds the quality of every
        base it counts in A, C, G or T.  16 B of device memory per kept base.  Refused once a row has added since
        pileup_enable() or pileup_reset(); while they are kept pileup_batch needs quals.  keep=False frees them and leaves the
        counters."""
        N.check(N.lib().dcn_anchor_map_pileup_keep_qualities(self._h, 1 if keep else 0))

    def pileup_fetch_qualities(self, record, start=0, n=None):
        """the quality sums of positions [start, start + n) of a record (n=None: to its end) -> np.uint32[n, 4], the columns
        PILEUP_A, C, G, T"""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        out = np.zeros((max(n, 1), 4), np.uint32)
        N.check(N.lib().dcn_anchor_map_pileup_fetch_qualities(self._h, int(record), start, n, _ptr(out)))
        return out[:n]

    def genotype(self, record, start=0, n=None, ploidy=2, min_depth=3, min_gq=20, min_qual=20, err_centi=477, het_centi=301):
        """Rules G1-G8 (the definition of a genotype is in include/deacon_hip.h) over positions [start, start + n) of a record
        (n=None: to its end) of a map that keeps quality sums -> (gt np.uint8[n], gq np.uint8[n], sites GENOTYPE_SITE_DTYPE[]).
        gt is the index of the best genotype in GENOTYPES' order (ploidy 1: A C G T), or GENOTYPE_NONE where the position is
        not called; gq its quality, 0 .. 99, either way; the sites are the called positions whose genotype is not the
        reference's, in ascending position.  The defaults are conventions, not measured optima.  One call with an estimate
        and, on DCN_ERR_CAPACITY, a second with the size the first reported."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        p = N.GenotypeParams(int(ploidy), int(min_depth), int(min_gq), int(min_qual), int(err_centi), int(het_centi), (C.c_uint32 * 2)(0, 0))
        gt, gq = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        n_sites = C.c_uint64()

        def call(cap):
            sites = np.zeros(max(cap, 1), GENOTYPE_SITE_DTYPE)
            rc = N.lib().dcn_anchor_map_genotype(self._h, C.byref(p), int(record), start, n, _ptr(gt), _ptr(gq), _ptr(sites) if cap else None,
                                                 cap, C.byref(n_sites))
            return rc, sites

        rc, sites = call(n // 64 + 64)
        if rc == N.DCN_ERR_CAPACITY:
            rc, sites = call(int(n_sites.value))
        N.check(rc)
        return gt[:n], gq[:n], sites[:int(n_sites.value)]

    def reference_blocks(self, record, start=0, n=None, breaks=None, gq_edges=(20, 40, 60, 80, 99), ploidy=2, min_depth=3, min_gq=20,
                         min_qual=20, err_centi=477, het_centi=301):
        """Rules B1-B9 (the definition of a reference block is in include/deacon_hip_blocks.h) over positions [start, start + n)
        of a record (n=None: to its end) of a map that keeps quality sums -> (cls np.uint8[n], blocks REFERENCE_BLOCK_DTYPE[]).
        cls is BLOCK_VARIANT at a genotype site and at every position of `breaks` (record positions inside the range, any
        order), BLOCK_NO_COVERAGE, BLOCK_UNCALLED, or BLOCK_REF + the number of gq_edges at or under the position's GQ; the
        blocks are the maximal runs of one class other than BLOCK_VARIANT, in ascending position.  The default edges are a
        convention, not a measured optimum.  One call with an estimate and, on DCN_ERR_CAPACITY, a second with the size the
        first reported."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        edges = [int(e) for e in gq_edges]
        if len(edges) > 16 or any(not 0 <= e <= 255 for e in edges):  # (what the struct can carry; which lists are allowed is the library's to say)
            raise ValueError("gq_edges does not fit dcn_block_params: at most 16 entries of 0..255 (the library allows 15 of 1..99)")
        p = N.BlockParams(int(ploidy), int(min_depth), int(min_gq), int(min_qual), int(err_centi), int(het_centi), len(edges), 0,
                          (C.c_uint8 * 16)(*edges))
        brk = np.ascontiguousarray(np.asarray([] if breaks is None else breaks, dtype=np.uint64).reshape(-1))
        cls = np.zeros(max(n, 1), np.uint8)
        n_blocks = C.c_uint64()

        def call(cap):
            blocks = np.zeros(max(cap, 1), REFERENCE_BLOCK_DTYPE)
            rc = N.lib().dcn_anchor_map_reference_blocks(self._h, C.byref(p), int(record), start, n, _ptr(brk) if len(brk) else None, len(brk),
                                                         _ptr(cls), _ptr(blocks) if cap else None, cap, C.byref(n_blocks))
            return rc, blocks

        rc, blocks = call(n // 64 + 64)
        if rc == N.DCN_ERR_CAPACITY:
            rc, blocks = call(int(n_blocks.value))
        N.check(rc)
        return cls[:n], blocks[:int(n_blocks.value)]

    def phase_sites(self, sites):
        """Rule H1 (dcn_anchor_map_phase_sites; the definition of a phase is in include/deacon_hip_phase.h): the map's list of
        heterozygous sites, PHASE_SITE_DTYPE[] strictly ascending in (record, pos), a0 != a1 columns of A C G T.  Replaces the
        list there was and zeroes every link; an empty list (or None) frees it.  The map must keep bases."""
        sites = np.zeros(0, PHASE_SITE_DTYPE) if sites is None else np.ascontiguousarray(sites)
        if sites.dtype != PHASE_SITE_DTYPE or sites.ndim != 1:
            raise ValueError("phase_sites: sites must be a one-dimensional PHASE_SITE_DTYPE array")
        N.check(N.lib().dcn_anchor_map_phase_sites(self._h, _ptr(sites) if len(sites) else None, len(sites)))

    def phase_info(self):
        """-> (sites, rows, rows_linking, link_adds): the sites of the list, the counted rows (rule P2) handed to
        Placer.phase_batch since the list was set, those that added to at least one link, and the link adds"""
        info = np.zeros(4, np.uint64)
        N.check(N.lib().dcn_anchor_map_phase_info(self._h, _ptr(info)))
        return tuple(int(v) for v in info)

    def phase_links(self, first=0, n=None):
        """the counters of sites [first, first + n) of the list (n=None: to its end) -> np.uint32[n, 4]: n00 n01 n10 n11 of
        the link from site s to site s + 1 (rule H3), 0 where there is none"""
        first = int(first)
        sites = self.phase_info()[0]
        if first < 0 or first > sites or (n is not None and int(n) < 0):
            raise ValueError("phase_links: first must lie in 0 .. %d (the sites of the list) and n must not be negative" % sites)
        n = sites - first if n is None else int(n)
        out = np.zeros((max(n, 1), 4), np.uint32)
        N.check(N.lib().dcn_anchor_map_phase_links(self._h, first, n, _ptr(out)))
        return out[:n]

    def phase_solve(self, min_reads=2, max_minor_permille=200):
        """Rules H5-H7 over the whole list (dcn_anchor_map_phase_solve) -> PHASE_RESULT_DTYPE[sites]: per site the position
        of its set's head, the four counters of its link to the next site, the index of its set, its haplotype bit and
        PHASE_HEAD / PHASE_JOINED.  Haplotype 1 carries allele a[hap]; a set of one site is unphased.  min_reads = 2 and
        max_minor_permille = 200 are conventions, not measured optima."""
        p = N.PhaseParams(int(min_reads), int(max_minor_permille), (C.c_uint32 * 2)(0, 0))
        n = self.phase_info()[0]
        out = np.zeros(max(n, 1), PHASE_RESULT_DTYPE)
        N.check(N.lib().dcn_anchor_map_phase_solve(self._h, C.byref(p), _ptr(out)))
        return out[:n]

    def duplicates_enable(self):
        """An empty duplicate set on the map (dcn_anchor_map_duplicates_enable; the definition of a duplicate is in
        include/deacon_hip.h); again changes nothing.  The map need not keep bases."""
        N.check(N.lib().dcn_anchor_map_duplicates_enable(self._h, 1))

    def duplicates_disable(self):
        N.check(N.lib().dcn_anchor_map_duplicates_enable(self._h, 0))

    def duplicates_reset(self):
        """the set empty and the ordinals back at 0"""
        N.check(N.lib().dcn_anchor_map_duplicates_reset(self._h))

    def duplicates_info(self):
        """-> (seen, keyed, keys): units handed in since the last reset, those with a key, the distinct keys; the number of
        duplicates so far is keyed - keys"""
        seen, keyed, keys = C.c_uint64(), C.c_uint64(), C.c_uint64()
        N.check(N.lib().dcn_anchor_map_duplicates_info(self._h, C.byref(seen), C.byref(keyed), C.byref(keys)))
        return int(seen.value), int(keyed.value), int(keys.value)

    def mark_duplicates(self, offsets, rows, row_offsets=None, paired=False, both_ends=False):
        """Rules D1-D7 over the rows of a batch (dcn_mark_duplicates_batch): offsets are the batch's (only the reads' lengths
        are taken from them), rows and row_offsets as Placer.verify_batch takes them.  A unit is a read, or with paired=True
        reads 2u and 2u + 1; its key is the unclipped 5' end (with both_ends also the 3' end) of the first placed row of each
        of its reads, and it is a duplicate when a unit handed in earlier since the last reset, in this call or a call before
        it, had the same key.  -> (dup np.uint8[units], first np.uint64[units]: the ordinal of the first unit with the key,
        2^64 - 1 for a unit without one)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = len(offsets) - 1
        rows = np.ascontiguousarray(rows)
        n_rows = len(rows)
        if row_offsets is not None:
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        n_units = n_reads // 2 if paired else n_reads
        dup, first = np.zeros(max(n_units, 1), np.uint8), np.zeros(max(n_units, 1), np.uint64)
        p = N.DuplicateParams(rows.dtype.itemsize, int(bool(paired)), int(bool(both_ends)), 0)
        N.check(N.lib().dcn_mark_duplicates_batch(self._h, _ptr(offsets), n_reads, C.byref(p), _ptr(row_offsets), _ptr(rows) if n_rows else None,
                                                  n_rows, _ptr(dup), _ptr(first), None))
        return dup[:n_units], first[:n_units]

    def insertions_info(self):
        """-> (events of the ledger, the sum of their lengths)"""
        n_events, n_bases = C.c_uint64(), C.c_uint64()
        N.check(N.lib().dcn_anchor_map_insertions_info(self._h, C.byref(n_events), C.byref(n_bases)))
        return int(n_events.value), int(n_bases.value)

    def _insertions(self, fn, head, dtype, n, estimate):
        """one call with an estimate and, on DCN_ERR_CAPACITY, a second with the sizes the first reported"""
        n_items, n_ins = C.c_uint64(), C.c_uint64()

        def call(cap, base_cap):
            items, bases = np.zeros(max(cap, 1), dtype), np.zeros(max(base_cap, 1), np.uint8)
            rc = fn(*head, _ptr(items) if cap else None, cap, _ptr(bases) if base_cap else None, base_cap, C.byref(n_items), C.byref(n_ins))
            return rc, items, bases

        rc, items, bases = call(estimate, 4 * estimate)
        if rc == N.DCN_ERR_CAPACITY:
            rc, items, bases = call(int(n_items.value), int(n_ins.value))
        N.check(rc)
        return items[:int(n_items.value)], bases[:int(n_ins.value)].tobytes()

    def insertions_fetch(self, record, start=0, n=None):
        """The events of the ledger anchored in [start, start + n) of a record (n=None: to its end), in the canonical order
        of rule L4 -> (INSERTION_DTYPE[], bases bytes): event e's bases are bases[e.bases_offset : e.bases_offset + e.len]."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        return self._insertions(N.lib().dcn_anchor_map_insertions_fetch, (self._h, int(record), start, n), INSERTION_DTYPE, n, n // 16 + 64)

    def insertions_call(self, record, start=0, n=None, min_depth=3, min_permille=500):
        """Rule L6 over [start, start + n) of a record -> (INSERTION_ALLELE_DTYPE[], bases bytes): per position with a called
        insertion its winning allele, its count and the events there, in ascending position.  The thresholds are
        pileup_call's, conventions and not measured optima."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        p = N.PileupCallParams(int(min_depth), int(min_permille), (C.c_uint32 * 2)(0, 0))
        return self._insertions(N.lib().dcn_anchor_map_insertions_call, (self._h, C.byref(p), int(record), start, n), INSERTION_ALLELE_DTYPE,
                                n, n // 64 + 64)

    def pileup_keep_deletions(self, keep=True):
        """A deletion ledger beside the pileup (dcn_anchor_map_pileup_keep_deletions; the definition of a deletion ledger is
        in include/deacon_hip.h): every D run of a row that Placer.pileup_batch adds also leaves (position, length, strand).
        Refused once a row has added since pileup_enable() or pileup_reset(); keep=False drops it and leaves the counters."""
        N.check(N.lib().dcn_anchor_map_pileup_keep_deletions(self._h, 1 if keep else 0))

    def pileup_left_align(self, on=True):
        """Left-align every row before it is piled up (dcn_anchor_map_pileup_left_align; the definition of a left-aligned
        placement is in include/deacon_hip.h): while on, Placer.pileup_batch adds the runs of rule N5 to the counters, the
        quality sums and both ledgers, so that a gap in a repeat lies at the repeat's near end.  Refused once a row has
        added since pileup_enable() or pileup_reset() (rule N8); pileup_disable() clears it."""
        N.check(N.lib().dcn_anchor_map_pileup_left_align(self._h, 1 if on else 0))

    def pileup_left_align_info(self):
        """-> dict of LEFT_ALIGN_INFO_DTYPE's five numbers, summed over the pileup_batch calls that ran with
        pileup_left_align() on since pileup_enable() or pileup_reset()"""
        info = np.zeros(1, LEFT_ALIGN_INFO_DTYPE)
        N.check(N.lib().dcn_anchor_map_pileup_left_align_info(self._h, _ptr(info)))
        return {name: int(info[name][0]) for name in LEFT_ALIGN_INFO_DTYPE.names}

    def deletions_info(self):
        """-> (events of the deletion ledger, the sum of their lengths)"""
        n_events, n_deleted = C.c_uint64(), C.c_uint64()
        N.check(N.lib().dcn_anchor_map_deletions_info(self._h, C.byref(n_events), C.byref(n_deleted)))
        return int(n_events.value), int(n_deleted.value)

    def deletions_fetch(self, record, start=0, n=None):
        """The events of the deletion ledger that begin in [start, start + n) of a record (n=None: to its end), in the
        canonical order of rule R4 -> DELETION_DTYPE[].  One call with an estimate and, on DCN_ERR_CAPACITY, a second with
        the size the first reported."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        n_events = C.c_uint64()

        def call(cap):
            events = np.zeros(max(cap, 1), DELETION_DTYPE)
            rc = N.lib().dcn_anchor_map_deletions_fetch(self._h, int(record), start, n, _ptr(events) if cap else None, cap, C.byref(n_events))
            return rc, events

        rc, events = call(n // 16 + 64)
        if rc == N.DCN_ERR_CAPACITY:
            rc, events = call(int(n_events.value))
        N.check(rc)
        return events[:int(n_events.value)]

    def indels_genotype(self, record, start=0, n=None, ploidy=2, min_depth=3, min_gq=20, min_qual=20, min_count=2, indel_centi=2000,
                        het_centi=301):
        """Rules I1-I8 (the definition of an indel genotype is in include/deacon_hip.h) over [start, start + n) of a record
        (n=None: to its end) of a map that keeps an insertion ledger, a deletion ledger or both -> (INDEL_SITE_DTYPE[], bases
        bytes): per position the winning insertion and the winning deletion that begin there, each genotyped against
        everything else, where the genotype is not the reference's; an insertion site's bases are
        bases[bases_offset : bases_offset + len].  The defaults are conventions, not measured optima."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        p = N.IndelParams(int(ploidy), int(min_depth), int(min_gq), int(min_qual), int(min_count), int(indel_centi), int(het_centi), 0)
        return self._insertions(N.lib().dcn_anchor_map_indels_genotype, (self._h, C.byref(p), int(record), start, n), INDEL_SITE_DTYPE, n,
                                n // 64 + 64)

    def pileup_keep_strands(self, keep=True):
        """Strand planes beside the pileup (dcn_anchor_map_pileup_keep_strands; the definition of strand evidence is in
        include/deacon_hip.h): four uint32 per base, RA RC RG RT, to which Placer.pileup_batch adds 1 for every base of a
        reverse row that it counts in A, C, G or T.  16 B of device memory per kept base.  Refused once a row has added since
        pileup_enable() or pileup_reset(); keep=False frees them and leaves the counters."""
        N.check(N.lib().dcn_anchor_map_pileup_keep_strands(self._h, 1 if keep else 0))

    def pileup_fetch_strands(self, record, start=0, n=None):
        """the reverse counters of positions [start, start + n) of a record (n=None: to its end) -> np.uint32[n, 4], the
        columns PILEUP_A, C, G, T; the forward count of a column is pileup_fetch's counter less this one"""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        out = np.zeros((max(n, 1), 4), np.uint32)
        N.check(N.lib().dcn_anchor_map_pileup_fetch_strands(self._h, int(record), start, n, _ptr(out)))
        return out[:n]

    def strand_evidence(self, record, queries, max_sb_centi=1083, min_alt_strand=1, min_strand_depth=3):
        """Rules S3-S6 (the definition of strand evidence is in include/deacon_hip.h) at the sites of `queries`, a
        STRAND_QUERY_DTYPE[] in any order, of a map that keeps strand planes -> STRAND_SITE_DTYPE[len(queries)]: the forward
        and reverse counts of the four columns (base queries), the 2 x 2 table, the score in hundredths of a chi-square and
        the flags STRAND_BIAS / STRAND_ONE_SIDED.  The defaults are conventions, not measured optima."""
        queries = np.ascontiguousarray(queries, dtype=STRAND_QUERY_DTYPE)
        p = N.StrandParams(int(max_sb_centi), int(min_alt_strand), int(min_strand_depth), 0)
        out = np.zeros(max(len(queries), 1), STRAND_SITE_DTYPE)
        N.check(N.lib().dcn_anchor_map_strand_evidence(self._h, C.byref(p), int(record), _ptr(queries) if len(queries) else None, len(queries),
                                                       _ptr(out)))
        return out[:len(queries)]

    def indels_strand(self, record, sites, bases=b""):
        """a_rev of rule S4 for the sites and bases that indels_genotype returned (dcn_anchor_map_indels_strand) ->
        np.uint32[len(sites)]: how many events of each site's winning allele came from reverse rows.  Needs the ledgers, not
        the strand planes."""
        sites = np.ascontiguousarray(sites, dtype=INDEL_SITE_DTYPE)
        bases = np.frombuffer(bytes(bases), np.uint8)
        out = np.zeros(max(len(sites), 1), np.uint32)
        N.check(N.lib().dcn_anchor_map_indels_strand(self._h, int(record), _ptr(sites) if len(sites) else None, len(sites),
                                                     _ptr(bases) if len(bases) else None, _ptr(out)))
        return out[:len(sites)]

    @staticmethod
    def strand_queries_of_genotypes(sites, ploidy=2):
        """the base queries of genotype()'s sites: ALT = the alleles of the site's genotype other than the record's base"""
        q = np.zeros(len(sites), STRAND_QUERY_DTYPE)
        gt = sites["gt"].astype(np.int64)
        if int(ploidy) == 2:  # rule G3's order: index y (y + 1) / 2 + x, x <= y
            y = ((np.sqrt(8 * gt + 1) - 1) // 2).astype(np.int64)
            x = gt - y * (y + 1) // 2
        else:
            x = y = gt
        ref = sites["ref_code"].astype(np.int64)
        q["pos"], q["ref_code"] = sites["pos"], ref
        q["alt_mask"] = ((1 << x) | (1 << y)) & ~(1 << ref) & 15
        return q

    @staticmethod
    def strand_queries_of_indels(sites, count_reverse):
        """the indel queries of indels_genotype()'s sites, with indels_strand()'s numbers"""
        q = np.zeros(len(sites), STRAND_QUERY_DTYPE)
        q["pos"], q["kind"], q["count"], q["count_reverse"] = sites["pos"], 1, sites["count"], count_reverse
        return q

    def genotype_strand(self, record, start=0, n=None, ploidy=2, min_depth=3, min_gq=20, min_qual=20, err_centi=477, het_centi=301,
                        max_sb_centi=1083, min_alt_strand=1, min_strand_depth=3):
        """genotype() and, for its sites, strand_evidence() -> (gt, gq, sites GENOTYPE_SITE_DTYPE[], STRAND_SITE_DTYPE[])"""
        gt, gq, sites = self.genotype(record, start, n, ploidy, min_depth, min_gq, min_qual, err_centi, het_centi)
        return gt, gq, sites, self.strand_evidence(record, self.strand_queries_of_genotypes(sites, ploidy), max_sb_centi, min_alt_strand,
                                                   min_strand_depth)

    def indels_genotype_strand(self, record, start=0, n=None, ploidy=2, min_depth=3, min_gq=20, min_qual=20, min_count=2, indel_centi=2000,
                               het_centi=301, max_sb_centi=1083, min_alt_strand=1, min_strand_depth=3):
        """indels_genotype() and, for its sites, indels_strand() and strand_evidence() -> (sites INDEL_SITE_DTYPE[], bases
        bytes, STRAND_SITE_DTYPE[])"""
        sites, bases = self.indels_genotype(record, start, n, ploidy, min_depth, min_gq, min_qual, min_count, indel_centi, het_centi)
        queries = self.strand_queries_of_indels(sites, self.indels_strand(record, sites, bases))
        return sites, bases, self.strand_evidence(record, queries, max_sb_centi, min_alt_strand, min_strand_depth)

    def consensus(self, record, start=0, n=None, min_depth=3, min_permille=500, fill_ref=False):
        """Rule L7 over [start, start + n) of a record -> bytes: per position the bases of a called front insertion, the
        called base (nothing for '-'; N, or with fill_ref the record's own base, where there is no call), the bases of a
        called insertion behind it.  Assembled here from pileup_call's characters and insertions_call's alleles: a linear
        copy, with numpy and no loop over bases."""
        start, n = int(start), self._to_end(record, start) if n is None else int(n)
        calls = np.frombuffer(self.pileup_call(record, start, n, min_depth, min_permille)[0], np.uint8)
        alleles, ins = self.insertions_call(record, start, n, min_depth, min_permille)
        ins = np.frombuffer(ins, np.uint8)
        own = calls
        if fill_ref:  # a position without a call: pileup_call writes N there, as it does nowhere else (N never wins)
            own = np.where(calls == ord("N"), np.frombuffer(self.fetch(record, start, n), np.uint8), calls)
        own_len = (own != ord("-")).astype(np.int64)
        q = (alleles["pos"].astype(np.int64) - start)
        front = (alleles["flags"] & N.INSERTION_FRONT) != 0
        before, behind = np.zeros(n, np.int64), np.zeros(n, np.int64)
        before[q[front]] = alleles["len"][front]
        behind[q[~front]] = alleles["len"][~front]
        begin = np.concatenate(([0], np.cumsum(before + own_len + behind)))  # where each position's output begins
        out = np.zeros(int(begin[-1]), np.uint8)
        keep = own_len.astype(bool)
        out[(begin[:-1] + before)[keep]] = own[keep]
        if len(alleles):
            dst0 = np.where(front, begin[:-1][q], (begin[:-1] + before + own_len)[q])  # where each allele's bases begin
            lens = alleles["len"].astype(np.int64)
            within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
            out[np.repeat(dst0, lens) + within] = ins[np.repeat(alleles["bases_offset"].astype(np.int64), lens) + within]
        return out.tobytes()

    def _to_end(self, record, start):
        """bases from `start` to the end of a record (the lengths of the records add() has taken are kept here)"""
        return self._record_lengths[int(record)] - int(start)

    def clone(self, device):
        h = C.c_void_p()
        N.check(N.lib().dcn_index_clone(self._h, int(device), C.byref(h)))
        return Index(h, int(device))

    def _context(self, n_bases, n_reads):
        """a context of the map's own, made on the first add and re-made larger for a longer batch"""
        have_bases, have_reads = (self._ctx.max_batch_bases, self._ctx.max_batch_reads) if self._ctx else (0, 0)
        if self._ctx and n_bases <= have_bases and n_reads <= have_reads:
            return self._ctx
        if self._ctx:
            self._ctx.close()
        self._ctx = _Context(self._h, max(int(n_bases), have_bases, 1 << 20), max(int(n_reads), have_reads, 1 << 10))
        return self._ctx

    def add(self, bases, offsets):
        """bases: concatenated ASCII; offsets[n_records+1] -> the number of the batch's first record"""
        bases, offsets, n = _batch(bases, offsets)
        first = C.c_uint32()
        ctx = self._context(int(offsets[-1]) if n > 0 else 0, n)
        N.check(N.lib().dcn_anchor_map_add(self._h, ctx._h, _ptr(bases) if len(bases) else None, _ptr(offsets), n, C.byref(first)))
        self._record_lengths += np.diff(offsets.astype(np.int64)).tolist() if n else []
        return first.value

    def add_records(self, records):
        bases, offsets = concat_reads(list(records))
        return self.add(bases, offsets)

    def info(self):
        """{records, keys, anchors, repeats}"""
        r, k, a, p = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        N.check(N.lib().dcn_anchor_map_info(self._h, C.byref(r), C.byref(k), C.byref(a), C.byref(p)))
        return {"records": r.value, "keys": k.value, "anchors": a.value, "repeats": p.value}

    def anchors(self):
        """(keys u64[], records u32[], positions u32[]) of the anchors, in arbitrary order"""
        n = C.c_uint64()
        rc = N.lib().dcn_anchor_map_anchors(self._h, None, None, None, 0, C.byref(n))
        if rc != N.DCN_ERR_CAPACITY:
            N.check(rc)
        cap = int(n.value)
        keys, rec, pos = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        N.check(N.lib().dcn_anchor_map_anchors(self._h, _ptr(keys), _ptr(rec), _ptr(pos), cap, C.byref(n)))
        return keys[:cap], rec[:cap], pos[:cap]

    def close(self):
        if getattr(self, "_ctx", None):
            self._ctx.close()
            self._ctx = None
        super().close()


class Placer(_Context):
    """Where on the reference each read lands (dcn_place_batch; the definition of a placement is in
    include/deacon_hip.h): a read's anchor hits vote on a diagonal band of band_bases bases; the best cell, with at least
    min_votes votes, gives the record, the strand and the extents on the read and on the record.  band_bases = 256 and
    min_votes = 2 are conventions (the 2 is the filter's -a 2), not measured optima.
    profile(): pack, plan, scan (minimizer dump), the probe sweep that marks positions and stores their anchors in the
    'distinct' slot and the vote in the 'finish' slot.  place_split_batch / place_split report up to max_placements
    placements per read with rival votes and a quality (dcn_place_split_batch); place_pair_batch / place_pairs place the
    two mates of a pair jointly (dcn_place_pair_batch); one Placer serves every kind of call alternately."""

    def __init__(self, anchor_map, max_batch_bases=1 << 26, max_batch_reads=1 << 20, band_bases=256, min_votes=2,
                 prefix_length=0):
        self.anchor_map = anchor_map
        self.band_bases = int(band_bases)
        self.min_votes = int(min_votes)
        self.prefix_length = int(prefix_length)
        super().__init__(anchor_map._h, max_batch_bases, max_batch_reads)

    def _params(self):
        return N.PlaceParams(self.band_bases, self.min_votes, self.prefix_length, (C.c_uint32 * 2)(0, 0))

    def place_batch(self, bases, offsets):
        """bases: concatenated ASCII; offsets[n_reads+1] -> PLACEMENT_DTYPE[n_reads]"""
        bases, offsets, n_reads = _batch(bases, offsets)
        out = np.zeros(max(n_reads, 1), PLACEMENT_DTYPE)
        p = self._params()
        N.check(N.lib().dcn_place_batch(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                        n_reads, C.byref(p), _ptr(out)))
        return out[:n_reads]

    def place(self, reads):
        bases, offsets = concat_reads(list(reads))
        return self.place_batch(bases, offsets)

    def place_split_batch(self, bases, offsets, max_placements=4, capacity=None):
        """Up to max_placements (1..8) placements per read, each from the anchor hits that no earlier one explained, with
        the votes of the strongest competing cell on the same stretch of the read and mapq = 60 * (votes - rival_votes)
        // votes (a convention, not a calibrated probability; dcn_place_split_batch, the definition is in
        include/deacon_hip.h).  bases: concatenated ASCII; offsets[n_reads+1] -> (place_offsets u64[n_reads+1],
        SPLIT_PLACEMENT_DTYPE[place_offsets[-1]], read_counts u32[n_reads, 2]): read r owns
        placements[place_offsets[r]:place_offsets[r+1]], ranks ascending, and read_counts[r] = (n_anchors, n_positions)
        also where it owns nothing.  capacity=None sizes the rows by n_reads * max_placements, which always suffices;
        a smaller capacity raises DeaconHipError(DCN_ERR_CAPACITY) when the batch has more."""
        bases, offsets, n_reads = _batch(bases, offsets)
        cap = n_reads * int(max_placements) if capacity is None else int(capacity)
        place_offsets = np.zeros(n_reads + 1, np.uint64)
        out = np.zeros(max(cap, 1), SPLIT_PLACEMENT_DTYPE)
        counts = np.zeros((max(n_reads, 1), 2), np.uint32)
        p = N.PlaceSplitParams(self.band_bases, self.min_votes, self.prefix_length, int(max_placements), (C.c_uint32 * 3)(0, 0, 0))
        N.check(N.lib().dcn_place_split_batch(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                              n_reads, C.byref(p), _ptr(place_offsets), _ptr(out) if cap else None, cap,
                                              _ptr(counts)))
        return place_offsets, out[:int(place_offsets[n_reads])], counts[:n_reads]

    def place_split(self, reads, max_placements=4):
        """-> per read the SPLIT_PLACEMENT_DTYPE rows it owns (none for an unplaced read)"""
        reads = list(reads)
        bases, offsets = concat_reads(reads)
        po, rows, _ = self.place_split_batch(bases, offsets, max_placements)
        return [rows[int(po[r]):int(po[r + 1])] for r in range(len(reads))]

    def place_pair_batch(self, bases, offsets, max_placements=4, max_insert=1000, hist_bin_bases=8, want_hist=True):
        """Reads 2u and 2u + 1 are the mates of pair u, placed jointly (dcn_place_pair_batch; the definition of a paired
        placement is in include/deacon_hip.h): a combination of one of the first max_placements rounds of each mate is
        concordant when the two lie on one record on opposite strands, the forward one begins before the reverse one
        ends and the template is at most max_insert bases; the concordant combination with the most votes makes the
        pair PROPER, and a mate with a single hit there is RESCUED.  Rival votes and mapq count the partner's votes in
        (a convention, not a calibrated probability; max_insert = 1000 and hist_bin_bases = 8 are conventions too).
        -> (PAIR_PLACEMENT_DTYPE[n_reads], one row per read with record == UNPLACED for an unplaced mate,
        u64[256] of proper pairs by tlen // hist_bin_bases with the last bin open-ended, or None with want_hist=False)"""
        bases, offsets, n_reads = _batch(bases, offsets)
        out = np.zeros(max(n_reads, 1), PAIR_PLACEMENT_DTYPE)
        hist = np.zeros(N.PAIR_HIST_BINS, np.uint64) if want_hist else None
        p = N.PlacePairParams(self.band_bases, self.min_votes, self.prefix_length, int(max_placements), int(max_insert),
                              int(hist_bin_bases), (C.c_uint32 * 3)(0, 0, 0))
        N.check(N.lib().dcn_place_pair_batch(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                             n_reads, C.byref(p), _ptr(out), _ptr(hist) if want_hist else None))
        return out[:n_reads], hist

    def verify_batch(self, bases, offsets, rows, row_offsets=None, max_edits=1023, max_permille=200):
        """The Levenshtein distance of each placement's read interval (reverse-complemented when the row says so) and its
        record interval, thresholded (dcn_verify_batch; the definition of a verified placement is in
        include/deacon_hip.h): edits = d when d <= E = min(max_edits, max(m, n) * max_permille // 1000), else VERIFY_OVER;
        VERIFY_UNPLACED for a row with record == UNPLACED.  The map must keep bases (AnchorMap(index, keep_bases=True)).
        rows: the rows of place_batch or place_pair_batch (row r belongs to read r), or those of place_split_batch with its
        place_offsets as row_offsets; the stride is the dtype's item size.  max_edits = 1023 and max_permille = 200 are
        conventions, not measured optima.  -> np.uint32[n_rows].  profile(): pack in its slot, the verify kernel in
        'finish'."""
        bases, offsets, n_reads = _batch(bases, offsets)
        rows = np.ascontiguousarray(rows)
        n_rows = len(rows)
        if row_offsets is not None:
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        edits = np.zeros(max(n_rows, 1), np.uint32)
        p = N.VerifyParams(int(max_edits), int(max_permille), rows.dtype.itemsize, 0)
        N.check(N.lib().dcn_verify_batch(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None, _ptr(offsets), n_reads,
                                         C.byref(p), _ptr(row_offsets), _ptr(rows) if n_rows else None, n_rows, _ptr(edits)))
        return edits[:n_rows]

    def align_batch(self, bases, offsets, rows, row_offsets=None, max_edits=1023, max_permille=200, capacity=None):
        """verify_batch, and the alignment of every row with edits = d <= E (dcn_align_batch; the definition of an aligned
        placement is in include/deacon_hip.h): -> (edits, cigar_offsets, cigar).  edits is verify_batch's; row r's runs
        are cigar[cigar_offsets[r]:cigar_offsets[r + 1]], each len << 4 | op with BAM's codes (I = 1, D = 2, '=' = 7,
        X = 8; cigar_string() prints them), in the record's direction; an OVER or UNPLACED row has none.  capacity=None:
        one call with an estimate and, on DCN_ERR_CAPACITY, a second with the size the first reported; a number: one call
        with that capacity, and the error is raised.  profile(): pack in its slot, both kernels, the scan and the
        gather in 'finish'."""
        return self._align_batch(None, bases, offsets, rows, row_offsets, max_edits, max_permille, capacity)

    def left_align_batch(self, bases, offsets, rows, row_offsets=None, max_edits=1023, max_permille=200, capacity=None):
        """align_batch with every aligned row left-aligned (dcn_left_align_batch; the definition of a left-aligned placement
        is in include/deacon_hip.h): a gap in a homopolymer or a tandem repeat lies at the repeat's near end in the record's
        direction, as VCF wants it, not at the far end where the walk back leaves it.  -> (edits, cigar_offsets, cigar,
        info): the first three as align_batch returns them, edits identical; info a dict of LEFT_ALIGN_INFO_DTYPE's five
        numbers for this call."""
        info = np.zeros(1, LEFT_ALIGN_INFO_DTYPE)
        out = self._align_batch(info, bases, offsets, rows, row_offsets, max_edits, max_permille, capacity)
        return out + ({name: int(info[name][0]) for name in LEFT_ALIGN_INFO_DTYPE.names},)

    def _align_batch(self, info, bases, offsets, rows, row_offsets, max_edits, max_permille, capacity):
        """align_batch (info None) and left_align_batch (a LEFT_ALIGN_INFO_DTYPE[1] that receives the totals)"""
        bases, offsets, n_reads = _batch(bases, offsets)
        rows = np.ascontiguousarray(rows)
        n_rows = len(rows)
        if row_offsets is not None:
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        edits = np.zeros(max(n_rows, 1), np.uint32)
        cigar_offsets = np.zeros(n_rows + 1, np.uint64)
        p = N.VerifyParams(int(max_edits), int(max_permille), rows.dtype.itemsize, 0)

        def call(cap):
            cigar = np.zeros(max(cap, 1), np.uint32)
            args = (self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None, _ptr(offsets), n_reads,
                    C.byref(p), _ptr(row_offsets), _ptr(rows) if n_rows else None, n_rows, _ptr(edits),
                    _ptr(cigar_offsets), _ptr(cigar) if cap else None, cap)
            rc = N.lib().dcn_align_batch(*args) if info is None else N.lib().dcn_left_align_batch(*args, _ptr(info))
            return rc, cigar

        rc, cigar = call(4 * n_rows + 64 if capacity is None else int(capacity))
        if rc == N.DCN_ERR_CAPACITY and capacity is None:
            rc, cigar = call(int(cigar_offsets[n_rows]))
        N.check(rc)
        return edits[:n_rows], cigar_offsets, cigar[:int(cigar_offsets[n_rows])]

    def pileup_batch(self, bases, offsets, rows, row_offsets=None, max_edits=1023, max_permille=200, select=None, quals=None,
                     min_base_qual=0, qual_offset=33):
        """align_batch's rows added to the anchor map's pileup (dcn_pileup_batch; the definition of a pileup is in
        include/deacon_hip.h): every row with an alignment adds one count per base of its record interval, in the column
        of the read's base there or in DEL, one in INS per inserted run, and REV beside each on the reverse strand.  The
        runs never leave the device.  select: an optional boolean mask over the rows; a row it leaves out is given as
        unplaced, in a copy (the caller's rows are not written).  -> (edits np.uint32[n_rows] as verify_batch returns
        them for the rows given, n_added).  The map needs AnchorMap.pileup_enable() first.  profile(): pack in its slot,
        everything else in 'finish'.
        quals: the base qualities, a uint8 array or bytes with one byte per base of the batch (dcn_pileup_batch_qual; the
        definition of a quality-aware pileup is in include/deacon_hip.h).  A base of quality byte - qual_offset below
        min_base_qual counts in N instead of its column, and a map with AnchorMap.pileup_keep_qualities() also sums the
        qualities of the counted bases.  What aligns does not change.  quals=None: the call without qualities, whatever
        min_base_qual and qual_offset say."""
        bases, offsets, n_reads = _batch(bases, offsets)
        rows = np.ascontiguousarray(rows)
        n_rows = len(rows)
        if quals is not None:
            if isinstance(quals, (bytes, bytearray, memoryview)):
                quals = np.frombuffer(quals, np.uint8)
            if not isinstance(quals, np.ndarray) or quals.dtype != np.uint8 or quals.shape != (len(bases),):
                raise ValueError("pileup_batch: quals must be uint8 or bytes with one byte per base of the batch")
            quals = np.ascontiguousarray(quals)
        if select is not None:
            select = np.asarray(select, bool)
            if select.shape != (n_rows,):
                raise ValueError("pileup_batch: select must hold one boolean per row")
            rows = rows.copy()
            rows["record"][~select] = UNPLACED
        if row_offsets is not None:
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        edits = np.zeros(max(n_rows, 1), np.uint32)
        n_added = C.c_uint64()
        p = N.VerifyParams(int(max_edits), int(max_permille), rows.dtype.itemsize, 0)
        if quals is not None:
            qp = N.PileupQualParams(int(qual_offset), int(min_base_qual), (C.c_uint32 * 2)(0, 0))
            N.check(N.lib().dcn_pileup_batch_qual(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None,
                                                  _ptr(quals) if len(quals) else None, _ptr(offsets), n_reads, C.byref(p), C.byref(qp),
                                                  _ptr(row_offsets), _ptr(rows) if n_rows else None, n_rows, _ptr(edits), C.byref(n_added)))
            return edits[:n_rows], int(n_added.value)
        N.check(N.lib().dcn_pileup_batch(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None, _ptr(offsets), n_reads,
                                         C.byref(p), _ptr(row_offsets), _ptr(rows) if n_rows else None, n_rows, _ptr(edits),
                                         C.byref(n_added)))
        return edits[:n_rows], int(n_added.value)

    def phase_batch(self, bases, offsets, rows, row_offsets=None, max_edits=1023, max_permille=200, select=None, quals=None,
                    min_base_qual=0, qual_offset=33):
        """pileup_batch's rows looked at once more, at the sites of AnchorMap.phase_sites alone (dcn_phase_batch; the
        definition of a phase is in include/deacon_hip_phase.h): every row with an alignment adds 1 to a counter of the
        link between two neighbouring sites when it shows one of the two alleles at both.  Arguments as for pileup_batch,
        and a row sees the column the pileup counted for it (quals, min_base_qual and the map's left-align switch
        included).  The map needs no pileup, and none is written.  -> (edits np.uint32[n_rows], n_linking: the rows of this
        call that added to at least one link)."""
        bases, offsets, n_reads = _batch(bases, offsets)
        rows = np.ascontiguousarray(rows)
        n_rows = len(rows)
        if quals is not None:
            if isinstance(quals, (bytes, bytearray, memoryview)):
                quals = np.frombuffer(quals, np.uint8)
            if not isinstance(quals, np.ndarray) or quals.dtype != np.uint8 or quals.shape != (len(bases),):
                raise ValueError("phase_batch: quals must be uint8 or bytes with one byte per base of the batch")
            quals = np.ascontiguousarray(quals)
            if len(quals) == 0:
                quals = None  # (a batch without bases has no quality to look at: the call without Q3)
        if select is not None:
            select = np.asarray(select, bool)
            if select.shape != (n_rows,):
                raise ValueError("phase_batch: select must hold one boolean per row")
            rows = rows.copy()
            rows["record"][~select] = UNPLACED
        if row_offsets is not None:
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        edits = np.zeros(max(n_rows, 1), np.uint32)
        n_linking = C.c_uint64()
        p = N.VerifyParams(int(max_edits), int(max_permille), rows.dtype.itemsize, 0)
        qp = None if quals is None else N.PileupQualParams(int(qual_offset), int(min_base_qual), (C.c_uint32 * 2)(0, 0))
        N.check(N.lib().dcn_phase_batch(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None,
                                        None if quals is None else _ptr(quals), _ptr(offsets), n_reads, C.byref(p),
                                        None if qp is None else C.byref(qp), _ptr(row_offsets), _ptr(rows) if n_rows else None, n_rows,
                                        _ptr(edits), C.byref(n_linking)))
        return edits[:n_rows], int(n_linking.value)

    def extend_batch(self, bases, offsets, rows, row_offsets=None, penalty=6, end_bonus=4, max_edits=1023):
        """Each placement carried over the two flanks of its read, the bases outside its outermost anchor hits
        (dcn_extend_batch; the definition of an extended placement is in include/deacon_hip.h): on either side the end
        that maximises read bases + record bases - penalty * edits, with end_bonus added for reaching the read's end and
        at most max_edits edits; what is left of the read is the soft clip.  rows, row_offsets: as for verify_batch.
        penalty = 6, end_bonus = 4 and max_edits = 1023 are conventions, not measured optima.
        -> (rows_extended, extension): a copy of `rows`, of the same dtype, with read_start, read_end, ref_start and
        ref_end replaced -- what verify_batch, align_batch and pileup_batch take next -- and EXTENSION_DTYPE[n_rows] with
        the same four and the edits of the left and the right flank, in the record's direction.  An unplaced row comes
        back as it was.  profile(): pack in its slot, the extend kernel in 'finish'."""
        bases, offsets, n_reads = _batch(bases, offsets)
        rows = np.ascontiguousarray(rows)
        n_rows = len(rows)
        if row_offsets is not None:
            row_offsets = np.ascontiguousarray(row_offsets, dtype=np.uint64)
        ext = np.zeros(max(n_rows, 1), EXTENSION_DTYPE)
        p = N.ExtendParams(int(penalty), int(end_bonus), int(max_edits), rows.dtype.itemsize, (C.c_uint32 * 2)(0, 0))
        N.check(N.lib().dcn_extend_batch(self._h, self.anchor_map._h, _ptr(bases) if len(bases) else None, _ptr(offsets), n_reads,
                                         C.byref(p), _ptr(row_offsets), _ptr(rows) if n_rows else None, n_rows, _ptr(ext)))
        ext = ext[:n_rows]
        rows_extended = rows.copy()
        for name in ("read_start", "read_end", "ref_start", "ref_end"):
            rows_extended[name] = ext[name]
        return rows_extended, ext

    def place_pairs(self, reads1, reads2, **kw):
        """the mates of two lists, interleaved -> place_pair_batch's result"""
        reads1, reads2 = list(reads1), list(reads2)
        if len(reads1) != len(reads2):
            raise ValueError("place_pairs: the two lists must have one mate each per pair")
        bases, offsets = concat_reads([m for pair in zip(reads1, reads2) for m in pair])
        return self.place_pair_batch(bases, offsets, **kw)


class FilterProcessor(_Context):
    """One pipeline context bound to an index: decides keep/drop for units (reads or pairs)."""

    def __init__(self, index, abs_threshold=2, rel_threshold=0.01, prefix_length=0, deplete=False,
                 max_batch_bases=1 << 26, max_batch_reads=1 << 20):
        self.index = index
        self.abs_threshold = int(abs_threshold)
        self.rel_threshold = float(rel_threshold)
        self.prefix_length = int(prefix_length)
        self.deplete = bool(deplete)
        super().__init__(index._h, max_batch_bases, max_batch_reads)

    # -- parameters -----------------------------------------------------------------------------------
    def _params(self):
        return Params(self.abs_threshold, self.rel_threshold, self.prefix_length, 1 if self.deplete else 0, 0)

    # -- the batch seam ---------------------------------------------------------------------------------
    def filter_batch(self, bases, offsets, unit_id=None, counts=True):
        """bases: concatenated ASCII; offsets[n_reads+1]; unit_id groups mates -> (keep bool[], hits, total).
        counts=False asks for the decisions only (returns just keep): the kernels may then stop probing a read once
        its decision is fixed, which is what `deacon filter` needs outside --debug."""
        bases, offsets, n_reads = _batch(bases, offsets)
        if unit_id is not None:
            unit_id = np.ascontiguousarray(unit_id, dtype=np.uint32)
            n_units = int(unit_id[-1]) + 1 if n_reads else 0
        else:
            n_units = n_reads
        keep = np.zeros(max(n_units, 1), np.uint8)
        p = self._params()
        if not counts:
            N.check(N.lib().dcn_filter_batch(self._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                             _ptr(unit_id), n_reads, C.byref(p), _ptr(keep), None, None))
            return keep[:n_units].astype(bool)
        hits = np.zeros(max(n_units, 1), np.uint32)
        total = np.zeros(max(n_units, 1), np.uint32)
        N.check(N.lib().dcn_filter_batch(self._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                         _ptr(unit_id), n_reads, C.byref(p), _ptr(keep), _ptr(hits), _ptr(total)))
        return keep[:n_units].astype(bool), hits[:n_units], total[:n_units]

    def _outputs(self, offsets, unit_id, counts, out):
        n_reads = len(offsets) - 1
        n_units = (int(unit_id[-1]) + 1 if n_reads else 0) if unit_id is not None else n_reads
        if out is not None:
            keep, hits, total = out
        else:
            keep = np.zeros(max(n_units, 1), np.uint8)
            hits = np.zeros(max(n_units, 1), np.uint32) if counts else None
            total = np.zeros(max(n_units, 1), np.uint32) if counts else None
        return n_reads, n_units, keep, hits, total

    def submit(self, bases, offsets, unit_id=None, counts=True, out=None):
        """dcn_filter_batch_submit: returns a PendingBatch; up to two may be in flight per processor.
        out = (keep u8[], hits u32[] | None, total u32[] | None) lets the caller supply (page-locked) result arrays."""
        bases, offsets, _ = _batch(bases, offsets)
        if unit_id is not None:
            unit_id = np.ascontiguousarray(unit_id, dtype=np.uint32)
        n_reads, n_units, keep, hits, total = self._outputs(offsets, unit_id, counts, out)
        p = self._params()
        t = C.c_uint64()
        N.check(N.lib().dcn_filter_batch_submit(self._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                                _ptr(unit_id), n_reads, C.byref(p), _ptr(keep), _ptr(hits),
                                                _ptr(total), C.byref(t)))
        return PendingBatch(self, t.value, n_units, keep, hits, total, (bases, offsets, unit_id, p))

    def submit_packed(self, packed, invmask, offsets, unit_id=None, counts=True, out=None):
        """dcn_filter_batch_packed_submit: the batch as a 2-bit stream + invalid mask (see pack_ascii)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        invmask = np.ascontiguousarray(invmask, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if unit_id is not None:
            unit_id = np.ascontiguousarray(unit_id, dtype=np.uint32)
        n_reads, n_units, keep, hits, total = self._outputs(offsets, unit_id, counts, out)
        g = (int(offsets[-1]) + 31) // 32 if n_reads else 0
        if len(packed) < 2 * g or len(invmask) < g:
            raise ValueError("packed / invmask must hold whole 32-base groups of the batch")
        p = self._params()
        t = C.c_uint64()
        N.check(N.lib().dcn_filter_batch_packed_submit(self._h, _ptr(packed), _ptr(invmask), _ptr(offsets),
                                                       _ptr(unit_id), n_reads, C.byref(p), _ptr(keep), _ptr(hits),
                                                       _ptr(total), C.byref(t)))
        return PendingBatch(self, t.value, n_units, keep, hits, total, (packed, invmask, offsets, unit_id, p))

    def filter_batch_packed(self, packed, invmask, offsets, unit_id=None, counts=True):
        """dcn_filter_batch_packed (blocking)."""
        return self.submit_packed(packed, invmask, offsets, unit_id, counts).wait()

    def filter_reads(self, reads, paired=False):
        """reads: list of sequences; paired=True: reads 2i and 2i+1 are the mates of pair i."""
        bases, offsets = concat_reads(reads)
        unit_id = (np.arange(len(reads), dtype=np.uint32) // 2) if paired else None
        return self.filter_batch(bases, offsets, unit_id)

    def filter_batch_device(self, d_bases, d_offsets, n_reads, n_bases, d_keep, d_hits=None, d_total=None,
                            d_unit_id=None, n_units=None):
        """Same computation on device-resident inputs; arguments are raw device pointers (ints).  Asynchronous:
        call synchronize() before reading the outputs."""
        p = self._params()
        if n_units is None:
            n_units = n_reads
        N.check(N.lib().dcn_filter_batch_device(self._h, d_bases, d_offsets, d_unit_id, n_reads, n_bases, n_units,
                                                C.byref(p), d_keep, d_hits, d_total))

    def last_batch_short(self):
        """True when the last batch synchronize() waited for was packed inside the scan kernel (a device batch of short
        unpaired reads, dcn_ctx_last_batch_short), False when it took the classic pack pass.  Same results either way.  Batches of
        filter_batch_device only: the host entry points do not change the answer."""
        v = C.c_uint32()
        N.check(N.lib().dcn_ctx_last_batch_short(self._h, C.byref(v)))
        return bool(v.value)

    def reserve_records(self, n_records):
        N.check(N.lib().dcn_ctx_reserve_records(self._h, int(n_records)))

    # -- the per-read seam of the reference ----------------------------------------------------------------
    def should_keep_sequence(self, seq):
        keep, hits, total = self.filter_reads([seq])
        return bool(keep[0]), int(hits[0]), int(total[0])

    def should_keep_pair(self, seq1, seq2):
        keep, hits, total = self.filter_reads([seq1, seq2], paired=True)
        return bool(keep[0]), int(hits[0]), int(total[0])

    # -- counters -------------------------------------------------------------------------------------------
    def reset_stats(self):
        N.check(N.lib().dcn_ctx_reset_stats(self._h))

    def set_profiling(self, enable=True):
        """True / 1: every stage; 2: the scan stage only (cheaper: two events per batch); False / 0: off"""
        N.check(N.lib().dcn_ctx_set_profiling(self._h, 2 if enable == 2 else (1 if enable else 0)))

    def summary(self, elapsed_seconds):
        """The numeric fields of FilterSummary (filter_common.rs:11-38; filled at local_filter.rs:780-821)."""
        s = self.stats()
        seqs_in, bp_in = s["total_seqs"], s["total_bp"]
        seqs_out, bp_out = seqs_in - s["filtered_seqs"], s["output_bp"]

        def prop(a, b):
            return a / b if b else 0.0

        return {
            "k": self.index.kmer_length, "w": self.index.window_size,
            "abs_threshold": self.abs_threshold, "rel_threshold": self.rel_threshold,
            "prefix_length": self.prefix_length, "deplete": self.deplete,
            "seqs_in": seqs_in, "seqs_out": seqs_out, "seqs_out_proportion": prop(seqs_out, seqs_in),
            "seqs_removed": s["filtered_seqs"], "seqs_removed_proportion": prop(s["filtered_seqs"], seqs_in),
            "bp_in": bp_in, "bp_out": bp_out, "bp_out_proportion": prop(bp_out, bp_in),
            "bp_removed": s["filtered_bp"], "bp_removed_proportion": prop(s["filtered_bp"], bp_in),
            "time": elapsed_seconds,
            "seqs_per_second": int(seqs_in / elapsed_seconds) if elapsed_seconds > 0 else 0,
            "bp_per_second": int(bp_in / elapsed_seconds) if elapsed_seconds > 0 else 0,
        }

    # -- minimizers (parity seam) ------------------------------------------------------------------------------
    def minimizer_hashes_batch(self, bases, offsets, prefix_length=None):
        """-> (out_offsets u64[n+1], hashes u64[], positions u32[]) for every read of the batch."""
        bases, offsets, n_reads = _batch(bases, offsets)
        pl = self.prefix_length if prefix_length is None else int(prefix_length)
        out_off = np.zeros(n_reads + 1, np.uint64)
        cap = max(int(len(bases)), 1)
        hashes = np.zeros(cap, np.uint64)
        pos = np.zeros(cap, np.uint32)
        N.check(N.lib().dcn_minimizer_hashes_batch(self._h, _ptr(bases) if len(bases) else None, _ptr(offsets),
                                                   n_reads, pl, _ptr(out_off), _ptr(hashes), _ptr(pos), cap))
        n = int(out_off[-1])
        return out_off, hashes[:n], pos[:n]

    def should_keep_hashes(self, hashes, hash_offsets):
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        hash_offsets = np.ascontiguousarray(hash_offsets, dtype=np.uint64)
        n_units = len(hash_offsets) - 1
        keep = np.zeros(max(n_units, 1), np.uint8)
        hits = np.zeros(max(n_units, 1), np.uint32)
        total = np.zeros(max(n_units, 1), np.uint32)
        p = self._params()
        N.check(N.lib().dcn_should_keep_hashes(self._h, _ptr(hashes) if len(hashes) else None, _ptr(hash_offsets),
                                               n_units, C.byref(p), _ptr(keep), _ptr(hits), _ptr(total)))
        return keep[:n_units].astype(bool), hits[:n_units], total[:n_units]


def merge_blocks(blocks):
    """Rule B6 (dcn_reference_blocks_merge; host only): REFERENCE_BLOCK_DTYPE[] in ascending position -> a new array in which
    touching blocks of one class are one.  Blocks that overlap or are out of order are an error."""
    out = np.array(blocks, dtype=REFERENCE_BLOCK_DTYPE, copy=True).reshape(-1)
    kept = C.c_uint64()
    N.check(N.lib().dcn_reference_blocks_merge(_ptr(out) if len(out) else None, len(out), C.byref(kept)))
    return out[:int(kept.value)]


def stats_allreduce(processors):
    """dcn_stats_allreduce: the six counters summed over several processors of this process."""
    arr = (C.c_void_p * len(processors))(*[p._h for p in processors])
    c = (C.c_uint64 * N.N_STATS)()
    N.check(N.lib().dcn_stats_allreduce(arr, len(processors), c))
    return dict(zip(N.STAT_NAMES, (int(x) for x in c)))


def get_minimizer_hashes_and_positions(processor, seq, prefix_length=0):
    """filter_common.rs:211-310 for one read -> (hashes u64[], positions u32[])."""
    bases, offsets = concat_reads([seq])
    _, h, p = processor.minimizer_hashes_batch(bases, offsets, prefix_length)
    return h, p


def _should_keep(processor, per_unit_hashes, abs_threshold, rel_threshold, deplete):
    lens = np.fromiter((len(h) for h in per_unit_hashes), dtype=np.uint64, count=len(per_unit_hashes))
    off = np.zeros(len(per_unit_hashes) + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = (np.concatenate([np.asarray(h, dtype=np.uint64) for h in per_unit_hashes])
            if len(per_unit_hashes) and off[-1] else np.zeros(0, np.uint64))
    saved = (processor.abs_threshold, processor.rel_threshold, processor.deplete)
    processor.abs_threshold, processor.rel_threshold, processor.deplete = int(abs_threshold), float(rel_threshold), bool(deplete)
    try:
        keep, hits, total = processor.should_keep_hashes(flat, off)
    finally:
        processor.abs_threshold, processor.rel_threshold, processor.deplete = saved
    return [(bool(k), int(h), int(t)) for k, h, t in zip(keep, hits, total)]


def unpaired_should_keep(processor, input_minimizers, abs_threshold, rel_threshold, deplete):
    """remote_filter.rs:230-264: one Vec<u64> of minimizer hashes per read -> [(keep, hits, total)]."""
    return _should_keep(processor, input_minimizers, abs_threshold, rel_threshold, deplete)


def paired_should_keep(processor, input_minimizers, abs_threshold, rel_threshold, deplete):
    """remote_filter.rs:266-301: one Vec<u64> per pair (both mates' hashes concatenated)."""
    return _should_keep(processor, input_minimizers, abs_threshold, rel_threshold, deplete)
