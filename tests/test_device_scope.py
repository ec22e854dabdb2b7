"""tests/device.py's on_device scope against a fake module that records its calls (no device, no library)."""
import numpy as np
import pytest

from tests.device import on_device


class FakeBuffer:
    def __init__(self, log, ident):
        self.log, self.ptr = log, ident

    def upload(self, arr):
        self.log.append(("upload", self.ptr))
        return self

    def free(self):
        self.log.append(("free", self.ptr))


class FakeLib:
    def __init__(self, log):
        self.log = log

    def pz_memset_d(self, handle, ptr, byte, nbytes):
        self.log.append(("memset", ptr, byte, nbytes))


class FakeModule:
    """records (name, *args) of every call; a name in `failing` raises after it is recorded"""

    def __init__(self, failing=()):
        self.log, self.failing, self.handle = [], set(failing), "handle"
        self.lib = FakeLib(self.log)

    def device_alloc(self, nbytes):
        self.log.append(("alloc", len([e for e in self.log if e[0] == "alloc"])))
        return FakeBuffer(self.log, self.log[-1][1])

    def __getattr__(self, name):
        if not name.startswith(("set_", "pin_key", "unpin_key")):
            raise AttributeError(name)

        def call(*args):
            self.log.append((name, *args))
            if name in self.failing:
                raise RuntimeError(name)
        return call


def names(log):
    return [e[0] for e in log]


def test_success_order_and_untouched_switches():
    hip = FakeModule()
    with on_device(hip, chunk=3, fuse=(False, True), timing=True) as dev:
        key = dev.upload(np.zeros(4, dtype=np.int64))
        out = dev.alloc(64)
        dev.pin(key, 1, 2, 3, 4)
        hip.log.append(("body",))
    assert hip.log == [("set_chunk", 3), ("set_fusion", False, True), ("set_kernel_timing", True),
                       ("alloc", 0), ("upload", 0), ("alloc", 1), ("memset", 1, 0x5A, 64), ("pin_key", 0, 1, 2, 3, 4), ("body",),
                       ("unpin_key", 0), ("set_kernel_timing", False), ("set_fusion", True, True), ("set_chunk", 0),
                       ("free", 0), ("free", 1)]
    assert out.ptr == 1
    assert not {"set_small_path", "set_margin_probe", "set_graphs"} & set(names(hip.log))


def test_every_switch_restores_to_its_default_and_no_switch_means_no_setter():
    hip = FakeModule()
    with on_device(hip, chunk=0, fuse=(True, True), small_path=False, graphs=False, timing=False, probe=True):
        mark = len(hip.log)
    assert hip.log[mark:] == [("set_margin_probe", False), ("set_kernel_timing", False), ("set_graphs", True), ("set_small_path", True),
                              ("set_fusion", True, True), ("set_chunk", 0)]
    hip = FakeModule()
    with on_device(hip) as dev:
        dev.alloc(8, poison=False)
    assert hip.log == [("alloc", 0), ("free", 0)]


def test_body_raises_everything_is_undone_once():
    hip = FakeModule()
    with pytest.raises(KeyError, match="body"):
        with on_device(hip, chunk=3, fuse=(False, False)) as dev:
            d_a = dev.upload(np.zeros(2))
            d_res = d_a                         # in place: one buffer under two names
            early = dev.alloc(16)
            d_k = dev.key(type("PMat", (), {"data": np.zeros(3)}))
            dev.pin(d_k, 1, 1, 2, 2)
            dev.pin(d_a, 1, 1, 2, 2)
            dev.free(early)
            mark = len(hip.log)
            raise KeyError("body")
    assert hip.log[mark:] == [("unpin_key", 0), ("unpin_key", 2), ("set_fusion", True, True), ("set_chunk", 0), ("free", 0), ("free", 2)]
    assert sorted(e[1] for e in hip.log if e[0] == "free") == [0, 1, 2] and d_res is d_a


@pytest.mark.parametrize("failing", ["unpin_key", "set_fusion"])
def test_body_error_wins_over_a_clean_up_error_and_the_later_steps_run(failing):
    hip = FakeModule()
    with pytest.raises(KeyError, match="body"):
        with on_device(hip, chunk=3, fuse=(False, False)) as dev:
            dev.pin(dev.alloc(8), 1, 1, 2, 2)
            dev.pin(dev.alloc(8), 1, 1, 2, 2)
            hip.failing = {failing}
            mark = len(hip.log)
            raise KeyError("body")
    assert hip.log[mark:] == [("unpin_key", 1), ("unpin_key", 0), ("set_fusion", True, True), ("set_chunk", 0), ("free", 0), ("free", 1)]


def test_clean_up_error_after_a_clean_body_propagates_and_the_later_steps_run():
    hip = FakeModule()
    with pytest.raises(RuntimeError, match="unpin_key"):
        with on_device(hip, chunk=3) as dev:
            dev.pin(dev.alloc(8), 1, 1, 2, 2)
            hip.failing = {"unpin_key"}
            mark = len(hip.log)
    assert hip.log[mark:] == [("unpin_key", 0), ("set_chunk", 0), ("free", 0)]


def test_a_setter_that_fails_on_entry_is_restored_with_the_ones_before_it():
    hip = FakeModule(failing={"set_small_path"})
    with pytest.raises(RuntimeError, match="set_small_path"):
        with on_device(hip, chunk=2, small_path=False, probe=True):
            raise AssertionError("the body must not run")
    assert hip.log == [("set_chunk", 2), ("set_small_path", False), ("set_small_path", True), ("set_chunk", 0)]
