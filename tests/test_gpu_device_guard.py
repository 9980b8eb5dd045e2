"""GPU, two devices: every C entry that makes HIP calls on a device of the caller's choosing
leaves the caller's own device current (csrc/lora_internal.h, DeviceGuard), and computes there
what it computes on device 0.

Device 0 is current throughout.  One tiny call of each family runs on device 1 - the integer, the
rational and the synthesis bank, a plan's demod, scan and device frame finder, the codec, the
profiling entries - and after each the current device is still 0 and the result equals, bit for
bit, that of the same call on device 0.  Skipped on a machine with one device."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TAPS = np.array([0.25, 0.5, 0.25], np.float32)


@pytest.fixture(scope="module")
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    import lora_phy_amd

    torch.cuda.set_device(0)
    return lora_phy_amd


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))


def raw_bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def on_both(call):
    """call(device index) -> a tuple of tensors, on device 1 and then on device 0, device 0 current
    before and after both; the two results compared bit for bit."""
    assert torch.cuda.current_device() == 0
    got = call(1)
    assert torch.cuda.current_device() == 0
    torch.cuda.synchronize(1)
    want = call(0)
    assert torch.cuda.current_device() == 0
    torch.cuda.synchronize(0)
    assert len(got) == len(want) and len(got) > 0
    for g, w in zip(got, want):
        assert g.device.index == 1 and w.device.index == 0
        assert g.shape == w.shape and g.dtype == w.dtype and g.numel() > 0
        assert torch.equal(raw_bits(g), raw_bits(w))


@pytest.mark.parametrize("interp,decim", [(1, 2), (2, 3)])
def test_down_converter_banks(amd, interp, decim):
    from lora_phy_amd import stream

    x = noise(64, 1)

    def call(d):
        chan = stream.Channelizer(decim=decim, taps=TAPS, period=8, steps=[1, 3], device=f"cuda:{d}", interp=interp)
        return (chan.run(x.to(f"cuda:{d}")),)

    on_both(call)


def test_synthesis_bank(amd):
    from lora_phy_amd import stream

    x = noise(16, 2).reshape(2, 8)

    def call(d):
        synth = stream.Synthesizer(interp=2, taps=TAPS, period=8, steps=[1, 3], device=f"cuda:{d}")
        return (synth.run(x.to(f"cuda:{d}")),)

    on_both(call)


def test_plan_demod_scan_find_and_profile(amd):
    from lora_phy_amd import _capi, stream

    sf, hop = 7, 64
    syms = torch.tensor([[77]], dtype=torch.int32)

    def call(d):
        dev = f"cuda:{d}"
        iq = amd.modulate(syms.to(dev), sf)          # one frame of 3 symbols: the sync word and one more
        assert torch.cuda.current_device() == 0 and iq.shape == (1, 3 << sf)
        plan = amd.DemodPlan(sf, device=dev)
        assert torch.cuda.current_device() == 0
        lib = _capi.lib()
        _capi.check(lib.lora_demod_profile_enable(plan._h, 1))
        assert torch.cuda.current_device() == 0
        res = plan.run(iq)
        assert torch.cuda.current_device() == 0
        stage, calls = (C.c_float * 3)(), C.c_int(0)
        _capi.check(lib.lora_demod_profile_read(plan._h, stage, C.byref(calls)))
        assert torch.cuda.current_device() == 0 and calls.value == 1
        _capi.check(lib.lora_demod_profile_enable(plan._h, 0))
        assert torch.cuda.current_device() == 0
        met = plan.scan(iq[0], hop)
        assert torch.cuda.current_device() == 0
        found = stream.find_frames_device(met, hop, sf, 1, 1)
        assert torch.cuda.current_device() == 0
        out = (iq, res.symbols, res.sync, res.cfo, res.time_offset, res.max_amp, met.power, met.power_avg, met.index,
               found.count, found.end)
        plan.close()
        assert torch.cuda.current_device() == 0
        return out

    on_both(call)


def test_codec_round_trip(amd):
    from lora_phy_amd import codec

    payload = torch.arange(8, dtype=torch.uint8) * 31

    def call(d):
        p = payload.to(f"cuda:{d}")
        s = codec.encode(p)
        assert torch.cuda.current_device() == 0
        back = codec.decode(s)
        assert torch.cuda.current_device() == 0
        assert torch.equal(back.payload.cpu(), payload)
        return (s, back.payload, back.errors)

    on_both(call)
