"""The plan lifecycle of ``stable_audio_tools._hip`` (``build_plan`` / ``plan_workspace`` / ``destroy_plan``), which the DiT, the codec
and both text encoders share, against a recording stand-in for the library: call order, clean-up after a failure, what the staging
tensors look like, the grow-only workspace.  No GPU and no native library."""
import pytest
import torch

KINDS = ["dit", "oobleck", "t5", "roberta"]


class FakeLib:
    """Records every ``sat_*`` call as (name, args); ``fail`` maps a call name to the return code of its ``fail_at``-th use."""

    def __init__(self, fail=None, fail_at=0, workspace=4096):
        self.calls, self.fail, self.fail_at, self.workspace = [], fail or {}, fail_at, workspace

    def sat_last_error(self):
        return b"recorded failure"

    def __getattr__(self, name):
        if not name.startswith("sat_"):
            raise AttributeError(name)

        def call(*args):
            seen = sum(1 for n, _ in self.calls if n == name)
            self.calls.append((name, args))
            if name.endswith("_workspace_bytes"):
                args[-1]._obj.value = self.workspace          # ctypes.byref(c_size_t)
            return self.fail[name] if name in self.fail and seen == self.fail_at else 0
        return call

    def names(self):
        return [n for n, _ in self.calls]


@pytest.fixture
def hip(monkeypatch):
    from stable_audio_tools import _hip

    def install(**kw):
        fake = FakeLib(**kw)
        monkeypatch.setattr(_hip, "_lib", fake)
        monkeypatch.setattr(_hip, "ptr", lambda t: t)          # the recording keeps the tensor itself
        monkeypatch.setattr(_hip, "stream", lambda: "stream")
        return _hip, fake
    return install


def _tensors():
    return {"a.weight": torch.arange(12, dtype=torch.float64).reshape(3, 4).t(),          # neither fp32 nor contiguous
            "b.bias": torch.ones(5, dtype=torch.float16),
            "c.gamma": torch.nn.Parameter(torch.full((2, 2), 3.0))}


@pytest.mark.parametrize("with_configure", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_build_plan_call_order_and_staging_tensors(hip, kind, with_configure):
    _hip, fake = hip()
    handle = object()
    tensors = _tensors()

    def create():
        fake.calls.append(("create", ()))
        return handle

    def configure(h):
        fake.calls.append(("configure", (h,)))

    got = _hip.build_plan(kind, create, tensors, "cpu", configure if with_configure else None)
    assert got is handle
    set_tensor = f"sat_{kind}_plan_set_tensor"
    assert fake.names() == ["create"] + ["configure"] * with_configure + [set_tensor] * 3 + [f"sat_{kind}_plan_finalize"]
    if with_configure:
        assert fake.calls[1][1] == (handle,)
    for (_, (h, name, t, numel)), (want_name, src) in zip(fake.calls[1 + with_configure:-1], tensors.items()):
        assert h is handle and name == want_name.encode() and numel == src.numel()
        assert t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and t.device.type == "cpu"
        assert torch.equal(t, src.detach().float())
    assert fake.calls[-1][1] == (handle, "stream")


@pytest.mark.parametrize("rc", [-3, -1])
@pytest.mark.parametrize("step,at", [("set_tensor", 0), ("set_tensor", 2), ("finalize", 0)])
@pytest.mark.parametrize("kind", KINDS)
def test_failed_build_destroys_the_plan_once(hip, kind, step, at, rc):
    _hip, fake = hip(fail={f"sat_{kind}_plan_{step}": rc}, fail_at=at)
    handle = object()
    result = []
    with pytest.raises(_hip.SatError, match=f"error {rc}: recorded failure"):
        result.append(_hip.build_plan(kind, lambda: handle, _tensors(), "cpu"))
    assert result == []
    destroys = [args for n, args in fake.calls if n == f"sat_{kind}_plan_destroy"]
    assert destroys == [(handle,)]
    assert fake.names()[-1] == f"sat_{kind}_plan_destroy"          # nothing touches the handle afterwards
    assert fake.names().count(f"sat_{kind}_plan_finalize") == (step == "finalize")


def test_failed_configure_destroys_the_plan_and_failed_create_has_nothing_to_destroy(hip):
    _hip, fake = hip()
    handle = object()

    def configure(h):
        raise _hip.SatError("configure refused")

    with pytest.raises(_hip.SatError, match="configure refused"):
        _hip.build_plan("dit", lambda: handle, _tensors(), "cpu", configure)
    assert fake.calls == [("sat_dit_plan_destroy", (handle,))]

    def create():
        raise _hip.SatError("create refused")

    fake.calls.clear()
    with pytest.raises(_hip.SatError, match="create refused"):
        _hip.build_plan("dit", create, _tensors(), "cpu")
    assert fake.calls == []


@pytest.mark.parametrize("kind", KINDS)
def test_destroy_plan(hip, kind):
    _hip, fake = hip()
    _hip.destroy_plan(kind, None)
    assert fake.calls == []
    handle = object()
    _hip.destroy_plan(kind, handle)
    assert fake.calls == [(f"sat_{kind}_plan_destroy", (handle,))]


@pytest.mark.parametrize("kind", KINDS)
def test_plan_workspace_grows_only(hip, kind):
    _hip, fake = hip(workspace=4096)
    handle = object()
    first = _hip.plan_workspace(kind, handle, None, "cpu", 2, 64)
    assert first.dtype == torch.uint8 and first.numel() == 4096 and first.device.type == "cpu"
    name, args = fake.calls[-1]
    assert name == f"sat_{kind}_workspace_bytes" and args[:3] == (handle, 2, 64)
    assert _hip.plan_workspace(kind, handle, first, torch.device("cpu"), 2, 64) is first
    fake.workspace = 1024                              # a smaller request keeps the larger buffer
    assert _hip.plan_workspace(kind, handle, first, "cpu", 1, 64) is first
    fake.workspace = 4097
    grown = _hip.plan_workspace(kind, handle, first, "cpu", 4, 64)
    assert grown is not first and grown.numel() == 4097
    fake.fail = {f"sat_{kind}_workspace_bytes": -5}
    fake.fail_at = len([n for n in fake.names() if n == f"sat_{kind}_workspace_bytes"])
    with pytest.raises(_hip.SatError):
        _hip.plan_workspace(kind, handle, grown, "cpu", 4, 64)


def test_same_device_resolves_the_current_cuda_device(monkeypatch):
    from stable_audio_tools import _hip
    D = torch.device
    current = [0]
    monkeypatch.setattr(torch.cuda, "current_device", lambda: current[0])
    assert D("cuda") != D("cuda:0")                      # what the helper is for
    assert _hip.same_device(D("cuda"), D("cuda:0")) and _hip.same_device(D("cuda:0"), D("cuda"))
    assert _hip.same_device("cuda", D("cuda")) and _hip.same_device(D("cuda:1"), "cuda:1")
    assert not _hip.same_device(D("cuda"), D("cuda:1")) and not _hip.same_device(D("cuda:0"), D("cuda:1"))
    assert not _hip.same_device(D("cpu"), D("cuda")) and _hip.same_device(D("cpu"), "cpu")
    current[0] = 1
    assert _hip.same_device(D("cuda"), D("cuda:1")) and not _hip.same_device(D("cuda"), D("cuda:0"))
