"""Every device allocation of the host runtime is released exactly once.

tests/alloc_balance_child.py runs one lifetime of three contexts (lanes regrown, a Galois key set, the
psum and the HPS digit-sum buffers, the host API's staging) in a fresh process with EXACTO_DEBUG_ALLOC=1
(DESIGN.md §3): the library logs every allocation and release with its pointer.  The log is replayed in
order here.  Nothing is read from the device's free-memory figure, which other processes change.
"""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = re.compile(r"^alloc-dbg (\w+) p=(\S+) ")
# allocation call -> the release call that must end it
PAIRS = {"hipMalloc": "hipFree", "hipMallocFromPoolAsync": "hipFreeAsync", "hipMallocAsync": "hipFreeAsync"}


def replay(log):
    """(allocations, errors, live): live maps each pointer still allocated to the release it waits for."""
    live, errors, allocations = {}, [], 0
    for no, line in enumerate(log.splitlines(), 1):
        m = RECORD.match(line)
        if not m:
            continue
        what, p = m.groups()
        if p in ("(nil)", "0", "0x0"):   # a zero-byte request: no block
            continue
        if what in PAIRS:
            if p in live:
                errors.append(f"line {no}: {what} returned {p}, which is still live")
            live[p] = PAIRS[what]
            allocations += 1
        elif what in PAIRS.values():
            if live.get(p) != what:
                errors.append(f"line {no}: {what} of {p}, " +
                              (f"which waits for {live[p]}" if p in live else "which is not live"))
            else:
                del live[p]
    return allocations, errors, live


def test_replay_sees_leaks_and_double_frees():
    log = ("alloc-dbg hipMalloc p=0x10 bytes=8 pool=(nil) stream=(nil) range=(nil)+0\n"
           "exacto-alloc pool 0x1 device 0 release threshold set ok, read back 0xffffffffffffffff\n"
           "alloc-dbg hipMallocFromPoolAsync p=0x20 bytes=8 pool=0x1 stream=0x2 range=(nil)+0\n"
           "alloc-dbg hipFree p=0x10 bytes=0 pool=(nil) stream=(nil) range=(nil)+0\n")
    assert replay(log) == (2, [], {"0x20": "hipFreeAsync"})
    _, errors, _ = replay(log + "alloc-dbg hipFree p=0x10 bytes=0 pool=(nil) stream=(nil) range=(nil)+0\n")
    assert len(errors) == 1 and "not live" in errors[0]
    _, errors, _ = replay(log + "alloc-dbg hipFree p=0x20 bytes=0 pool=(nil) stream=(nil) range=(nil)+0\n")
    assert len(errors) == 1 and "waits for hipFreeAsync" in errors[0]


@pytest.mark.gpu
def test_every_allocation_is_released_once(gpu_available):
    env = dict(os.environ)
    env["EXACTO_DEBUG_ALLOC"] = "1"
    env.pop("EXACTO_LEAK_CTX", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "alloc_balance_child.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    allocations, errors, live = replay(r.stderr)
    # the workspaces of two lanes alone are more than this: the log was there and was parsed
    assert allocations > 50, allocations
    assert not errors, errors[:10]
    assert not live, sorted(live.items())[:10]
