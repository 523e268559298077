"""lap_amd/serve_cache.py on the CPU: the rules a captured graph rests on (records rebuilt in place, never during a capture, all
of them reached by `refresh()` with sources ahead of their dependents), on plain tensors and a hand-moved version counter."""
import types

import pytest
import torch

from lap_amd.serve_cache import ServeCache


class _Rig:
    """A store over a fake parameter `w` with a version counter, a log of waits and builds, and a switchable capture flag."""

    def __init__(self):
        self.params = types.SimpleNamespace(version=0)
        self.w = torch.arange(4.0)
        self.log = []
        self.capturing = False
        self.store = ServeCache(self.params, "cpu", lambda unit: self.log.append(("wait", unit)), lambda: self.capturing)

    def update(self, w):
        self.w = w
        self.params.version += 1

    def double(self, unit="u"):
        """2 w, rebuilt in place."""
        def build(old):
            self.log.append(("build", "double", old is not None))
            new = 2 * self.w
            return new if old is None else old.copy_(new)
        return self.store.get(("double",), unit, build)

    def plus_one(self):
        """double + 1: a record made from another record."""
        def build(old):
            self.log.append(("build", "plus_one", old is not None))
            new = self.double() + 1
            return new if old is None else old.copy_(new)
        return self.store.get(("dep", "plus_one"), None, build)


def test_hit_calls_neither_build_nor_wait():
    r = _Rig()
    first = r.double()
    assert r.log == [("wait", "u"), ("build", "double", False)]
    r.log.clear()
    assert r.double() is first and r.log == []


def test_version_bump_rebuilds_once_in_place_after_one_wait():
    r = _Rig()
    first = r.double()
    ptr = first.data_ptr()
    r.update(torch.ones(4))
    r.log.clear()
    second = r.double()
    assert r.log == [("wait", "u"), ("build", "double", True)]       # one wait, before the one build, which got the old value
    assert second.data_ptr() == ptr and torch.equal(second, torch.full((4,), 2.0))
    assert r.double() is second and len(r.log) == 2


def test_no_unit_no_wait():
    r = _Rig()
    r.double(unit=None)
    assert r.log == [("build", "double", False)]


def test_rebuild_at_another_address_raises():
    r = _Rig()
    build = lambda old: 2 * r.w              # a fresh tensor on every call
    r.store.get(("fresh",), None, build)
    r.update(torch.ones(4))
    with pytest.raises(RuntimeError, match="another address"):
        r.store.get(("fresh",), None, build)
    with pytest.raises(RuntimeError, match="another address"):
        r.store.refresh()
    r = _Rig()
    pair = lambda old: (old[0], torch.zeros(2)) if old is not None else (torch.zeros(2), torch.zeros(2))
    r.store.get(("pair",), None, pair)      # one moved tensor of a tuple is enough
    r.update(torch.ones(4))
    with pytest.raises(RuntimeError, match="another address"):
        r.store.get(("pair",), None, pair)


@pytest.mark.parametrize("dependent_first", [True, False])
def test_refresh_rebuilds_a_source_before_its_dependent(dependent_first):
    r = _Rig()
    if dependent_first:
        dep, src = r.plus_one(), r.double()       # the source is first requested INSIDE the dependent's build
    else:
        src, dep = r.double(), r.plus_one()
    assert list(r.store.entries()) == [("double",), ("dep", "plus_one")]
    ptrs = (src.data_ptr(), dep.data_ptr())
    r.update(torch.full((4,), 5.0))
    r.log.clear()
    r.store.refresh()
    assert [e for e in r.log if e[0] == "build"] == [("build", "double", True), ("build", "plus_one", True)]
    assert r.store.stale() == []
    assert torch.equal(src, torch.full((4,), 10.0)) and torch.equal(dep, torch.full((4,), 11.0))     # the new source, not the old
    assert (r.double().data_ptr(), r.plus_one().data_ptr()) == ptrs
    assert r.store.entries("dep") == {"plus_one": dep}


def test_refresh_builds_nothing_that_is_current_and_creates_nothing():
    r = _Rig()
    r.store.refresh()
    assert r.log == [] and r.store.entries() == {}
    r.plus_one()
    r.log.clear()
    r.store.refresh()
    assert r.log == [] and list(r.store.entries()) == [("double",), ("dep", "plus_one")]


def test_no_build_inside_a_capture():
    r = _Rig()
    cur = r.double()
    r.capturing = True
    assert r.double() is cur                                      # a current record is served
    with pytest.raises(RuntimeError, match="stale inside a stream capture"):
        r.plus_one()                                              # a miss
    r.update(torch.ones(4))
    r.log.clear()
    with pytest.raises(RuntimeError, match="stale inside a stream capture"):
        r.double()                                                # a stale record
    with pytest.raises(RuntimeError, match="stale inside a stream capture"):
        r.store.refresh()
    assert r.log == [] and list(r.store.entries()) == [("double",)]
    r.capturing = False
    assert torch.equal(r.double(), torch.full((4,), 2.0))


def test_cpu_model_has_one_store_and_refresh_creates_nothing():
    from lap_amd.model import LAP
    from lap_amd.params import ParamStore
    from tests.common import debug_model_cfg

    cfg = debug_model_cfg()
    model = LAP(cfg, device="cpu", store=ParamStore(cfg, "cpu", with_optimizer=False, with_ema=False, with_grads=False))
    for old in ("_merged_w", "_dec_w8", "_prefill_pw", "_packed_w", "_mods_cache"):
        assert not hasattr(model, old), old
    model.refresh_serve_caches()
    model.refresh_serve_caches(10)
    assert model.serving_cache.entries() == {} and not hasattr(model, "_mods_cache")
