"""engine._TowerEngine, the host-side base of the five tower engines, without a GPU: the workspace cache (one rule for every engine: WS_KEEP
unpinned entries beside the newest, a workspace asked for under graph capture is never dropped) and the pixel check."""
import pytest
import torch

from law_of_vision_representation_in_mllms_amd import engine
from law_of_vision_representation_in_mllms_amd import vit_weights as VW


class Stub(engine._TowerEngine):
    """The base with a host "allocation"; the device only says "cuda" so that the capture question is asked at all (nothing touches a GPU)."""

    def __init__(self, keep, pixel_dtypes=None, side=28):
        super().__init__(None, VW.tiny_spec("clip", image_size=side), "cuda:0")
        self.WS_KEEP = keep
        if pixel_dtypes is not None:
            self.PIXEL_DTYPES = pixel_dtypes
        self.asked = []

    def _workspace_bytes(self, B):
        self.asked.append(B)
        return 8 * B

    def _allocate(self, nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8)


@pytest.fixture
def capturing(monkeypatch):
    state = {"on": False}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["on"])
    return state


def settings():
    """WS_KEEP as each engine class sets it."""
    got = {c.__name__: c.WS_KEEP for c in (engine.VitEngine, engine.VitEngineF32, engine.ConvNextEngine, engine.SamEngine)}
    assert got == {"VitEngine": 5, "VitEngineF32": 5, "ConvNextEngine": 5, "SamEngine": 0}
    return sorted(got.items())


def test_the_five_engines_share_the_base_and_its_one_cache():
    for cls in (engine.VitEngine, engine.VitEngineF32, engine.VitEngineCPU, engine.ConvNextEngine, engine.SamEngine):
        assert issubclass(cls, engine._TowerEngine)
        assert cls.workspace is engine._TowerEngine.workspace and cls._pixels is engine._TowerEngine._pixels
    settings()


def test_cache_keeps_ws_keep_entries_beside_the_newest(capturing):
    e = Stub(5)
    held = {b: e.workspace(b) for b in range(1, 9)}
    assert list(e._ws) == [3, 4, 5, 6, 7, 8] and not e._pinned
    assert all(e._ws[b] is held[b] and held[b].numel() == 8 * b for b in e._ws)
    assert e.workspace(5) is held[5] and e.asked == list(range(1, 9))          # a held size: the same object, nothing is sized again
    assert e.workspace(1) is not held[1] and list(e._ws) == [4, 5, 6, 7, 8, 1]  # a dropped one is made anew, the oldest goes
    e = Stub(0)
    for b in range(1, 9):
        ws = e.workspace(b)
        assert list(e._ws) == [b] and e._ws[b] is ws
    assert e.workspace(8) is ws


@pytest.mark.parametrize("name,keep", settings())
def test_a_workspace_asked_for_under_capture_is_never_dropped(capturing, name, keep):
    e = Stub(keep)
    e.workspace(40)
    capturing["on"] = True
    pinned = e.workspace(3)
    again = e.workspace(40)                                  # a resident one a capture asks for is pinned as well
    capturing["on"] = False
    assert e._pinned == {3, 40}
    for b in range(10, 20):
        e.workspace(b)
        assert e._ws[3] is pinned and e._ws[40] is again
    assert e.workspace(3) is pinned and e._pinned == {3, 40}
    assert [b for b in e._ws if b not in e._pinned] == list(range(10, 20))[-(keep + 1):]


def test_pixel_check_refuses_what_is_not_the_towers_input():
    e = Stub(5)
    for shape in ((3, 28, 28), (2, 4, 28, 28), (2, 3, 28, 21), (2, 3, 21, 28), (2, 3, 35, 35)):
        with pytest.raises(ValueError, match="doesn't match tower") as err:
            e._pixels(torch.zeros(shape))
        assert str(err.value) == f"Input image size {shape} doesn't match tower (28*28)."


def test_pixel_dtype_rules():
    e = Stub(5)
    e.device = torch.device("cpu")
    assert engine.VitEngine.PIXEL_DTYPES == engine.ConvNextEngine.PIXEL_DTYPES == engine.SamEngine.PIXEL_DTYPES == (torch.float32, torch.bfloat16)
    assert engine.VitEngineF32.PIXEL_DTYPES == engine.VitEngineCPU.PIXEL_DTYPES == (torch.float32,)
    px = torch.arange(2 * 3 * 28 * 28).reshape(2, 3, 28, 28) % 251
    for dtype, want in ((torch.uint8, torch.float32), (torch.float16, torch.float32), (torch.float64, torch.float32),
                        (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)):
        got = e._pixels(px.to(dtype))
        assert got.dtype == want and got.is_contiguous() and torch.equal(got.double(), px.to(dtype).double())
    f = Stub(5, (torch.float32,))                            # the fp32 engine and the host twin: everything becomes fp32
    f.device = torch.device("cpu")
    assert all(f._pixels(px.to(d)).dtype == torch.float32 for d in (torch.uint8, torch.float16, torch.bfloat16, torch.float32))
    strided = px.float().transpose(2, 3)
    assert not strided.is_contiguous() and e._pixels(strided).is_contiguous()


def test_state_index_keeps_each_engines_message():
    e = Stub(5)
    e.n_layers = 3
    assert [e._state(n, "m") for n in (None, 0, 3)] == [3, 0, 3]
    for n in (-1, 4):
        with pytest.raises(ValueError, match="^n_layers out of range$"):
            e._state(n, "n_layers out of range")
