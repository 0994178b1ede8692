"""Python restatements of the set table's group function (dcn_group_of, dcn_internal.h) and of the workgroup
classification kernel's hash partition (dcn_cls_partition, dcn_classify.h).  test_gpu_classify_seams.py builds its
adversarial inputs with them (keys with a chosen home group, hashes that crowd one partition); if either drifted from
the C++ the GPU tests would still pass but stop reaching the seams they aim at, so a host-only build of the headers pins
them here (no GPU needed)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deacon-server_amd", "csrc")

_GOLD32 = 0x9E3779B1
_GOLD64 = 0x9E3779B97F4A7C15
_M32 = np.uint64(0xFFFFFFFF)


def _rotl32(x, r):
    x = np.asarray(x, np.uint64) & _M32
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & _M32


def group_bits(n_groups):
    b = 0
    while (1 << b) < n_groups:
        b += 1
    return b


def group_of(keys, n_groups):
    """dcn_group_of(key, 32 - log2(n_groups), n_groups - 1) of a u64 array"""
    keys = np.asarray(keys, np.uint64)
    b = group_bits(n_groups)
    if b == 0:
        return np.zeros(len(keys), np.uint64)
    lo, hi = keys & _M32, keys >> np.uint64(32)
    with np.errstate(over="ignore"):
        x = ((lo ^ _rotl32(hi, 15)) * np.uint64(_GOLD32)) & _M32
    return (x >> np.uint64(32 - b)) & np.uint64(n_groups - 1)


def key_in_group(rng, g, n_groups, count):
    """count distinct non-zero keys whose home group among n_groups is g: dcn_group_of inverted (random hi, a 32-bit x
    with g in its top bits, lo = x * inverse(0x9E3779B1) ^ rotl32(hi, 15))"""
    b = group_bits(n_groups)
    inv = pow(_GOLD32, -1, 1 << 32)
    out = set()
    while len(out) < count:
        hi = int(rng.integers(1, 1 << 32))
        x = (g << (32 - b)) | int(rng.integers(0, 1 << (32 - b)))
        rot = ((hi << 15) | (hi >> 17)) & 0xFFFFFFFF
        lo = ((x * inv) & 0xFFFFFFFF) ^ rot
        out.add((hi << 32) | lo)
    return np.array(sorted(out), np.uint64)


def mix_hi32(h):
    """the top 32 bits of h * 0x9E3779B97F4A7C15 (mod 2^64)"""
    with np.errstate(over="ignore"):
        return (np.asarray(h, np.uint64) * np.uint64(_GOLD64)) >> np.uint64(32)


def partition(h, P):
    """dcn_cls_partition(h, P) of a u64 array: umulhi(mix_hi32(h), P)"""
    return (mix_hi32(h) * np.uint64(P)) >> np.uint64(32)


def test_replicas_match_the_headers(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "hash_replica_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(rocm, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "hash_replica_test.cpp"), "-o", str(exe)])
    rng = np.random.default_rng(2024)
    keys = np.concatenate([
        rng.integers(0, 2**63, 9000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 9000, dtype=np.uint64),
        rng.integers(0, 1 << 32, 900, dtype=np.uint64),  # hi = 0
        np.array([0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1, _GOLD64], np.uint64),
    ])
    for b, g in ((6, 0), (6, 63), (12, 4095), (17, 77777)):
        keys = np.concatenate([keys, key_in_group(rng, g, 1 << b, 20)])
    bits = [0, 6, 7, 11, 16, 20, 31]
    parts = [1, 2, 3, 4, 5, 7, 8, 10, 16, 1000, 2**31, 2**32 - 1]
    kf = tmp_path / "keys.txt"
    kf.write_text("".join(f"{int(k):x}\n" for k in keys))
    out = subprocess.run([str(exe), str(kf), *map(str, bits), "--", *map(str, parts)], check=True, capture_output=True,
                         text=True).stdout
    got = np.array([[int(v) for v in ln.split()] for ln in out.splitlines()], np.uint64)
    assert got.shape == (len(keys), len(bits) + len(parts))
    for c, b in enumerate(bits):
        assert got[:, c].tolist() == group_of(keys, 1 << b).tolist(), ("group", b)
    for c, P in enumerate(parts):
        assert got[:, len(bits) + c].tolist() == partition(keys, P).tolist(), ("partition", P)
    # the constructed keys land where they were aimed
    for b, g in ((6, 0), (6, 63), (12, 4095), (17, 77777)):
        ks = key_in_group(np.random.default_rng(b), g, 1 << b, 50)
        assert set(group_of(ks, 1 << b).tolist()) == {g}
