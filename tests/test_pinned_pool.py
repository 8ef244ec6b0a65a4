"""The page-locked block pool of boofcv_amd/api.py (_PinnedPool), without a GPU: each test runs in a child process whose _lib.load() returns
a fake library that hands out ctypes buffers from bhip_host_alloc and logs every bhip_host_free."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAKE_LIB = """
import ctypes as C, sys, types
from boofcv_amd import _lib, api

class FakeLib:
    def __init__(self):
        self.blocks = {}   # address -> ctypes buffer (kept alive: a freed block is never reused)
        self.freed = []
    def bhip_host_alloc(self, ctx, size, out):
        buf = C.create_string_buffer(size)
        self.blocks[C.addressof(buf)] = buf
        out._obj.value = C.addressof(buf)
        return _lib.BHIP_OK
    def bhip_host_free(self, p):
        self.freed.append(p.value)
        print("FREED", p.value, flush=True)
        return _lib.BHIP_OK

fake = FakeLib()
_lib.load = lambda: fake
ctx = types.SimpleNamespace(_h=1)
Pool = api._PinnedPool
"""


def _child(code, timeout=120):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", FAKE_LIB + code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_concurrent_release_keeps_the_pooled_byte_count():
    """Many threads take and release blocks at the same time: afterwards _pooled is the sum of the size classes sitting in _free."""
    r = _child("""
import threading, numpy as np
sys.setswitchinterval(1e-6)   # switch threads as often as possible: an unguarded read-modify-write loses updates
sizes = [100, 5000, 7000, 20000, 70000]
start = threading.Barrier(16)
def worker(k):
    start.wait()
    for i in range(2000):
        arrs = [Pool.arrays(ctx, [((sizes[(k + i + j) % len(sizes)],), np.uint8)]) for j in range(3)]
        del arrs   # the blocks go back to the pool from this thread
threads = [threading.Thread(target=worker, args=(k,)) for k in range(16)]
for t in threads: t.start()
for t in threads: t.join()
held = sum(size * len(lst) for size, lst in Pool._free.items())
addrs = [a for lst in Pool._free.values() for a in lst]
assert len(addrs) == len(set(addrs)), "a block sits in the pool twice"
assert Pool._pooled == held, (Pool._pooled, held)
assert held > 0 and not fake.freed
print("ok", held, len(fake.blocks))
""")
    assert r.returncode == 0, r.stdout + r.stderr
    assert any(line.startswith("ok") for line in r.stdout.splitlines()), r.stdout   # (the exit hook's FREED lines follow)


def test_block_alive_at_exit_is_never_freed():
    """A block still referenced by a numpy array when the interpreter exits stays allocated (the runtime reclaims it); a block sitting in
    the pool is freed by the exit hook."""
    r = _child("""
import numpy as np
live = Pool.arrays(ctx, [((1000,), np.float64)])[0]
live[:] = 1.0
released = Pool.arrays(ctx, [((10,), np.float64)])[0]
addr_released = released.ctypes.data
del released
print("LIVE", live.ctypes.data, flush=True)
print("POOLED", addr_released, flush=True)
""")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [line.split() for line in r.stdout.splitlines()]
    live = [int(w[1]) for w in lines if w[0] == "LIVE"]
    pooled = [int(w[1]) for w in lines if w[0] == "POOLED"]
    freed = [int(w[1]) for w in lines if w[0] == "FREED"]
    assert len(live) == 1 and len(pooled) == 1
    assert pooled[0] in freed, "the exit hook did not free the pooled block"
    assert live[0] not in freed, "a block still referenced by a live array was freed at exit"
