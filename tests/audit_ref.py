"""numpy restatement of audited exits (the definition is in include/mmee.h): the selection hash, the delivered / keep logic of one exit on top
of exit_stage_ref's decide, and the number of documents active at every exit of an audited forward.  The oracle of tests/test_host_audit.py
and tests/test_gpu_audit.py, written from the header's text, not from the kernel."""
import numpy as np

from . import exit_stage_ref as R

M32 = np.uint64(0xFFFFFFFF)


def cut_of(fraction):
    """floor(fraction 2^32 + 0.5) in [0, 2^32]."""
    assert 0.0 <= fraction <= 1.0
    return int(np.floor(np.float64(fraction) * 4294967296.0 + 0.5))


def hash32(slot, seed):
    """x = (uint32)slot * 0x9E3779B1 ^ seed through murmur3's fmix32; uint64 arrays holding 32-bit values."""
    x = (np.asarray(slot, np.int64).astype(np.uint64) & M32) * np.uint64(0x9E3779B1) & M32
    x = x ^ np.uint64(seed & 0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = x * np.uint64(0x85EBCA6B) & M32
    x = x ^ (x >> np.uint64(13))
    x = x * np.uint64(0xC2B2AE35) & M32
    return x ^ (x >> np.uint64(16))


def selected(cut, seed, slot):
    return hash32(slot, seed) < np.uint64(cut)


def mask(B, fraction, seed=0, slot_base=0):
    return selected(cut_of(fraction), seed, np.arange(B) + slot_base)


def audit_decide(stage, leave, delivered, *, cut, seed, slot_base, exit_index, is_final):
    """The audit on top of one exit's decision.  `leave` (n,) bool: the decision of exit_stage_ref.decide_ref for the stage's documents (the
    final exit: everybody); `delivered` [B] ints by original slot as they are before the launch (anything at exit 0: not read).
    Returns writes (n,): who gets out_logits / out_exit / out_conf here; keep (n,): who is in the next stage; delivered [B] after the launch
    (entries of slots outside the stage untouched); next: exit_stage_ref's next stage of `keep`."""
    o = np.asarray(stage["doc_orig"], np.int64)
    leave = np.asarray(leave, bool)
    was = np.zeros(stage["n"], bool) if exit_index == 0 else np.asarray(delivered)[o] != 0
    sel = selected(cut, seed, o + slot_base)
    now = was | (leave & sel & (not is_final))
    writes = leave & ~was
    keep = np.zeros(stage["n"], bool) if is_final else (~leave | now)
    out = np.array(delivered, np.int64, copy=True)
    if exit_index == 0:
        out[o] = now
    else:
        out[o[now != was]] = 1
    return dict(writes=writes, keep=keep, delivered=out, next=R._next_stage(stage, keep, ""))


def active_at_exit(exits, audited, E1):
    """#{exit_i >= e} + #{audited_i and exit_i < e} for e = 0 .. E1-1: what stage_counts() reports of an audited forward."""
    exits, audited = np.asarray(exits), np.asarray(audited, bool)
    return [int((exits >= e).sum() + (audited & (exits < e)).sum()) for e in range(E1)]
