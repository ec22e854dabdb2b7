"""Shared support of the GPU tests (tests/ only): the `mods` fixture, prepared keys, and the scope that puts a shared Module back.

A test file's Module is shared by every test of the file, so whatever one test sets on it - a chunk size, the fusion switches, a pinned
key - must be undone when that test fails as well; `on_device` does that once for all of them."""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mods():
    """n -> (RefModule(n), Module(n)), one pair per ring degree and per requesting test file."""
    from oracle.ref import RefModule
    from poulpy_amd.hal import Module
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = (RefModule(n), Module(n))
        return cache[n]
    return get


def prepared_key(ref, hip, mat):
    """`mat` (a MatZnx) prepared for the oracle and for the device: (pr, ph)."""
    shape = (mat.rows, mat.cols_in, mat.cols_out, mat.size)
    pr, ph = ref.vmp_pmat_alloc(*shape), hip.vmp_pmat_alloc(*shape)
    ref.vmp_prepare(pr, mat)
    hip.vmp_prepare(ph, mat)
    return pr, ph


# switch -> (setter, the value the tests leave it at); set in this order, restored in the reverse one
_SWITCHES = {
    "chunk": ("set_chunk", (0,)),
    "fuse": ("set_fusion", (True, True)),
    "small_path": ("set_small_path", (True,)),
    "graphs": ("set_graphs", (True,)),
    "timing": ("set_kernel_timing", (False,)),
    "probe": ("set_margin_probe", (False,)),
}


class _Scope:
    def __init__(self, hip):
        self.hip = hip
        self._set, self._pins, self._bufs = [], [], []

    def alloc(self, nbytes, poison=True):
        """A device buffer, 0x5A in every byte unless `poison` is off (an output must be written in full to compare equal)."""
        buf = self.hip.device_alloc(nbytes)
        self._bufs.append(buf)
        if poison:
            self.hip.lib.pz_memset_d(self.hip.handle, buf.ptr, 0x5A, nbytes)
        return buf

    def upload(self, array):
        array = np.ascontiguousarray(array)
        return self.alloc(array.nbytes, poison=False).upload(array)

    def key(self, ph):
        """The data of a prepared key (VmpPMat) on the device."""
        return self.upload(ph.data)

    def pin(self, buf, rows, cols_in, cols_out, size):
        ptr = getattr(buf, "ptr", buf)
        self.hip.pin_key(ptr, rows, cols_in, cols_out, size)
        self._pins.append(ptr)

    def free(self, buf):
        """Release `buf` before the scope ends."""
        self._bufs.remove(buf)
        buf.free()

    def _switch(self, switches):
        for name, (setter, _) in _SWITCHES.items():
            value = switches.pop(name, None)
            if value is not None:
                self._set.append(name)      # before the call: a setter that failed half-way is restored too
                getattr(self.hip, setter)(*(value if name == "fuse" else (value,)))
        assert not switches, f"unknown switches {sorted(switches)}"

    def _close(self):
        """Unpin, restore, free - every step runs whatever the ones before it did; returns the first error."""
        steps = [lambda p=p: self.hip.unpin_key(p) for p in reversed(self._pins)]
        steps += [lambda s=_SWITCHES[name]: getattr(self.hip, s[0])(*s[1]) for name in reversed(self._set)]
        steps += [buf.free for buf in self._bufs]
        self._pins, self._set, self._bufs = [], [], []
        first = None
        for step in steps:
            try:
                step()
            except Exception as e:
                first = first or e
        return first


@contextmanager
def on_device(hip, **switches):
    """with on_device(hip, chunk=, fuse=, small_path=, graphs=, timing=, probe=) as dev: the module switches named (and no other) are set
    for the body; `dev` hands out device buffers and pins keys.  On exit, raised or not: every pin is dropped, every switch named is put
    back to its default, every buffer is freed.  An error of the body wins over one of the clean-up (that one is dropped, it is mostly
    a consequence); after a clean body a clean-up error is raised."""
    dev = _Scope(hip)
    try:
        dev._switch(switches)
        yield dev
    except BaseException:
        dev._close()
        raise
    err = dev._close()
    if err is not None:
        raise err
