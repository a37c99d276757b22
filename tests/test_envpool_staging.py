"""EnvPool native staging (csrc/stager.{h,cc}): a thread of the pool copies
each finished batch out of the shared-memory segment into caller-supplied
ping-pong slots.

The env is deterministic. From its first step() on, every field is a function
of (env index, batch index, step count): the test sends each env its own
index as the action. The very first result comes from reset(), before any
action, so there the env is identified by the order in which its worker
created it, which the test can compute too.
"""
import gc
import itertools
import os
import signal
import threading
import time

import numpy as np
import pytest
import torch

import moolib_amd

FRAME = (3, 5)


def _ident_fields(ident, n, frame_shape):
    numel = int(np.prod(frame_shape))
    frame = ((ident * 31 + n * 7 + np.arange(numel)) % 256).astype(np.uint8)
    return {
        "frame": frame.reshape(frame_shape),
        "vec": np.array([ident, n], dtype=np.float32),
    }


class IndexedEnv:
    def __init__(self, creation_index, frame_shape):
        self.ident = 10000 + creation_index
        self.n = 0
        self.frame_shape = frame_shape

    def reset(self):
        return _ident_fields(self.ident, self.n, self.frame_shape)

    def step(self, action):
        self.ident = int(action)
        self.n += 1
        reward = float(self.ident) + 0.5 * self.n
        done = (self.ident + self.n) % 4 == 0
        return _ident_fields(self.ident, self.n, self.frame_shape), reward, done, {}


def make_factory(frame_shape=FRAME):
    calls = itertools.count()  # forked with each worker: a per-process index
    return lambda: IndexedEnv(next(calls), frame_shape)


def actions_for(B, b):
    return torch.arange(B, dtype=torch.int64) + 100 * b


def expected(B, W, b, n, frame_shape=FRAME):
    """What batch b's result must hold after n steps (n = 0: the reset)."""
    W = min(W, B)
    out = {
        "frame": torch.empty((B, *frame_shape), dtype=torch.uint8),
        "vec": torch.empty((B, 2), dtype=torch.float32),
        "reward": torch.zeros(B, dtype=torch.float32),
        "done": torch.zeros(B, dtype=torch.bool),
    }
    for e in range(B):
        if n == 0:
            # worker w = e % W creates its envs batch by batch, in row order
            owned = len(range(e % W, B, W))
            ident = 10000 + b * owned + e // W
        else:
            ident = e + 100 * b
            out["reward"][e] = float(ident) + 0.5 * n
            out["done"][e] = (ident + n) % 4 == 0
        f = _ident_fields(ident, n, frame_shape)
        out["frame"][e] = torch.from_numpy(f["frame"])
        out["vec"][e] = torch.from_numpy(f["vec"])
    return out


def make_slots(B, batches, frame_shape=FRAME, pin=False, num_slots=2):
    def one():
        d = {
            "frame": torch.full((B, *frame_shape), 0xEE, dtype=torch.uint8),
            "vec": torch.full((B, 2), -1.0),
            "reward": torch.full((B,), -1.0),
            "done": torch.zeros(B, dtype=torch.bool),
        }
        return {k: t.pin_memory() for k, t in d.items()} if pin else d

    return [[one() for _ in range(num_slots)] for _ in range(batches)]


def assert_fields_equal(got, want, what):
    assert set(got.keys()) == set(want.keys()), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k)


def native_threads():
    return len(os.listdir("/proc/self/task"))


def wait_for(cond, seconds):
    t0 = time.time()
    while not cond() and time.time() - t0 < seconds:
        time.sleep(0.002)
    return cond()


def close_within(holder, seconds=10.0):
    """Drop the last reference to the pool on a thread; it must not hang."""

    def closer():
        holder.clear()
        gc.collect()

    t = threading.Thread(target=closer, daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), "closing the pool hung"


@pytest.mark.parametrize("B,W,batches", [(5, 2, 2), (1, 1, 1), (7, 3, 2), (8, 8, 1)])
def test_staged_contents(B, W, batches):
    pool = moolib_amd.EnvPool(make_factory(), num_processes=W, batch_size=B, num_batches=batches)
    slots = make_slots(B, batches)
    pool.enable_staging(slots)
    assert pool.staging_enabled()
    ref_pool = moolib_amd.EnvPool(
        make_factory(), num_processes=W, batch_size=B, num_batches=batches
    )
    held = [None] * batches
    for n in range(25):
        futs = [pool.step(b, actions_for(B, b)) for b in range(batches)]
        for b in range(batches):
            out = futs[b].result()
            slot = pool.staged_slot(b)
            assert out is slots[b][slot]
            assert_fields_equal(out, expected(B, W, b, n), (b, n))
            if n == 0:
                view = ref_pool.step(b, actions_for(B, b)).result()
                assert_fields_equal(out, view, ("shm view", b))
            # like the training loop: a slot goes back at the batch's next result
            if held[b] is not None:
                pool.release(b, held[b])
            held[b] = slot
    holder = [pool, ref_pool]
    del pool, ref_pool
    close_within(holder)


def test_ping_pong_and_slot_reuse():
    B, W = 4, 2
    pool = moolib_amd.EnvPool(make_factory(), num_processes=W, batch_size=B, num_batches=1)
    slots = make_slots(B, 1)
    pool.enable_staging(slots)
    seen = []
    for n in range(2):
        out = pool.step(0, actions_for(B, 0)).result()
        seen.append(pool.staged_slot(0))
        assert_fields_equal(out, expected(B, W, 0, n), n)
    assert seen == [0, 1]
    frozen = [{k: t.clone() for k, t in s.items()} for s in slots[0]]

    # both slots are still the consumer's: the third step cannot be staged
    fut = pool.step(0, actions_for(B, 0))
    t0 = time.time()
    while time.time() - t0 < 0.5:
        assert not pool.poll(0)
        time.sleep(0.02)
    for s in range(2):
        assert_fields_equal(slots[0][s], frozen[s], ("unreleased slot", s))

    pool.release(0, 0)
    assert wait_for(lambda: pool.poll(0), 10.0)
    out = fut.result()
    assert pool.staged_slot(0) == 0
    assert_fields_equal(out, expected(B, W, 0, 2), "after release")
    assert_fields_equal(slots[0][1], frozen[1], "slot 1 still held")
    assert not pool.poll(0)  # consumed

    with pytest.raises(RuntimeError, match="bad batch or slot"):
        pool.release(0, 2)  # no such slot
    pool.release(0, 1)
    with pytest.raises(RuntimeError, match="release"):
        pool.release(0, 1)  # already handed back
    # alternation continues
    for n in range(3, 7):
        out = pool.step(0, actions_for(B, 0)).result()
        assert pool.staged_slot(0) == n % 2
        assert_fields_equal(out, expected(B, W, 0, n), n)
        pool.release(0, (n + 1) % 2)


def test_enable_staging_rejects_bad_calls():
    B = 3
    pool = moolib_amd.EnvPool(make_factory(), num_processes=2, batch_size=B, num_batches=1)
    with pytest.raises(RuntimeError, match="slot"):
        pool.enable_staging(make_slots(B, 1, num_slots=1))
    with pytest.raises(RuntimeError, match="contiguous"):
        bad = make_slots(B, 1)
        bad[0][0]["vec"] = torch.zeros(2, B).t()
        pool.enable_staging(bad)
    fut = pool.step(0, actions_for(B, 0))
    with pytest.raises(RuntimeError, match="in flight"):
        pool.enable_staging(make_slots(B, 1))
    fut.result()
    # between a consumed result and the next step it is valid; a slot whose
    # shape differs from the result's is reported by the next result
    wrong = make_slots(B + 1, 1)
    pool.enable_staging(wrong)
    with pytest.raises(RuntimeError, match="shape or dtype"):
        pool.step(0, actions_for(B, 0)).result()
    holder = [pool]
    del pool
    close_within(holder)


class FailsAtStep3Env(IndexedEnv):
    def step(self, action):
        if self.n == 2:
            raise RuntimeError("env exploded at step 3")
        return super().step(action)


class PidEnv:
    def reset(self):
        return np.array([os.getpid()], dtype=np.int64)

    def step(self, action):
        return np.array([os.getpid()], dtype=np.int64), 0.0, False, {}


def test_env_error_surfaces_and_pool_closes():
    B = 4
    pool = moolib_amd.EnvPool(
        lambda: FailsAtStep3Env(0, FRAME), num_processes=2, batch_size=B, num_batches=1
    )
    pool.enable_staging(make_slots(B, 1))
    for n in range(3):  # the reset and two good steps
        pool.step(0, actions_for(B, 0)).result()
        pool.release(0, pool.staged_slot(0))
    fut = pool.step(0, actions_for(B, 0))
    t0 = time.time()
    with pytest.raises(moolib_amd.RpcError, match=r"worker \d+ .*exploded at step 3"):
        fut.result()
    assert time.time() - t0 < 5.0
    assert pool.poll(0)  # a failure counts as "would not block"
    holder = [pool, fut]
    del pool, fut
    close_within(holder)


def test_killed_worker_surfaces_and_pool_closes():
    B = 2
    pool = moolib_amd.EnvPool(PidEnv, num_processes=2, batch_size=B, num_batches=1)
    slots = [
        [
            {
                "state": torch.zeros(B, 1, dtype=torch.int64),
                "reward": torch.zeros(B),
                "done": torch.zeros(B, dtype=torch.bool),
            }
            for _ in range(2)
        ]
    ]
    pool.enable_staging(slots)
    out = pool.step(0, torch.zeros(B, dtype=torch.int64)).result()
    pool.release(0, pool.staged_slot(0))
    pids = out["state"][:, 0].tolist()
    assert pids[0] != pids[1] and os.getpid() not in pids
    os.kill(pids[1], signal.SIGKILL)
    fut = pool.step(0, torch.zeros(B, dtype=torch.int64))
    t0 = time.time()
    with pytest.raises(moolib_amd.RpcError, match=r"worker 1 died"):
        fut.result()
    assert time.time() - t0 < 5.0
    holder = [pool, fut]
    del pool, fut
    close_within(holder)


def test_staging_is_off_by_default():
    torch.zeros(4).sum()  # let torch start whatever threads it starts lazily
    B = 4
    before = native_threads()
    pool = moolib_amd.EnvPool(make_factory(), num_processes=2, batch_size=B, num_batches=2)
    assert not pool.staging_enabled()
    region = pool.shared_buffer()
    lo, hi = region.data_ptr(), region.data_ptr() + region.numel()
    for n in range(3):
        for b in range(2):
            out = pool.step(b, actions_for(B, b)).result()
            assert_fields_equal(out, expected(B, 2, b, n), (b, n))
            for t in out.values():
                assert lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= hi
    assert native_threads() == before  # no stager thread
    with pytest.raises(RuntimeError, match="not enabled"):
        pool.staged_slot(0)
    with pytest.raises(RuntimeError, match="not enabled"):
        pool.release(0, 0)
    # the probe does see the thread once staging is on
    pool.enable_staging(make_slots(B, 2))
    assert native_threads() == before + 1
    out = pool.step(0, actions_for(B, 0)).result()
    assert not (lo <= out["frame"].data_ptr() < hi)
    assert_fields_equal(out, expected(B, 2, 0, 3), "staged after views")
    holder = [pool]
    del pool, region, out, t
    close_within(holder)
    assert native_threads() == before


@pytest.mark.gpu
def test_pinned_slots_to_device_like_the_training_loop():
    """Pinned slots -> persistent device buffers on a side stream with events,
    the protocol of ImpalaPeer._issue_h2d, for 30 steps."""
    B, W, batches, shape = 4, 2, 2, (4, 84, 84)
    pool = moolib_amd.EnvPool(
        make_factory(shape), num_processes=W, batch_size=B, num_batches=batches
    )
    slots = make_slots(B, batches, shape, pin=True)
    assert all(t.is_pinned() for per in slots for s in per for t in s.values())
    pool.enable_staging(slots)
    dev = "cuda:0"
    h2d = torch.cuda.Stream()
    staged = [{k: torch.empty_like(t, device=dev) for k, t in per[0].items()} for per in slots]
    slot_events = [[torch.cuda.Event() for _ in range(2)] for _ in range(batches)]
    consumed = [torch.cuda.Event() for _ in range(batches)]
    unreleased = [None] * batches
    want = [[expected(B, W, b, n, shape) for n in range(30)] for b in range(batches)]
    futs = [pool.step(b, actions_for(B, b)) for b in range(batches)]
    for n in range(30):
        for b in range(batches):
            assert wait_for(lambda: pool.poll(b), 30.0)
            out = futs[b].result()
            if unreleased[b] is not None:
                slot, ev = unreleased[b]
                if not ev.query():
                    ev.synchronize()
                pool.release(b, slot)
            slot = pool.staged_slot(b)
            assert slot == n % 2
            ev = slot_events[b][slot]
            unreleased[b] = (slot, ev)
            h2d.wait_event(consumed[b])
            with torch.cuda.stream(h2d):
                for k, t in out.items():
                    staged[b][k].copy_(t, non_blocking=True)
                ev.record()
            # the CPU side of the act (EnvBatchState.update reads the slot)
            assert torch.equal(out["reward"], want[b][n]["reward"])
            futs[b] = pool.step(b, actions_for(B, b))
            # the compute stream's read of the device buffers
            torch.cuda.current_stream().wait_event(ev)
            got = {k: t.clone() for k, t in staged[b].items()}
            consumed[b].record()
            assert_fields_equal({k: t.cpu() for k, t in got.items()}, want[b][n], (b, n))
    for b in range(batches):
        futs[b].result()
    torch.cuda.synchronize()
    holder = [pool]
    del pool, futs
    close_within(holder)
