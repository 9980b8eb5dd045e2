"""GPU modulation: lora_mod_batch wrapper and the LoRaMod block."""
from __future__ import annotations

from typing import Optional

import torch

from . import _capi
from .demod import _require_cuda, _stream_handle


def modulate(symbols: torch.Tensor, sf: int, osr: int = 1, bw: int = 125000,
             amplitude: float = 1.0, sync: int = 0x12, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lora_modulate (LoRaMod.cpp:8-43) for a [F, S] (or [S]) uint16/int CUDA tensor.

    Returns complex64 [F, (S+2)*N*osr] (or 1-D): two sync up-chirps, then one
    up-chirp per symbol, phase-continuous within each frame.  `out`: a contiguous
    complex64 tensor of that shape on the symbols' device to write into (no allocation).
    """
    _require_cuda(symbols, "symbols")
    squeeze = symbols.dim() == 1
    s = symbols.unsqueeze(0) if squeeze else symbols
    if s.dtype != torch.uint16:
        s = s.to(torch.int32).to(torch.uint16)
    s = s.contiguous()
    F, S = s.shape
    osr = int(osr) if osr else 1
    per = (S + 2) * (1 << int(sf)) * osr
    if out is None:
        out = torch.empty((F, per), dtype=torch.complex64, device=s.device)
    else:
        want = (per,) if squeeze else (F, per)
        if (tuple(out.shape) != want or out.dtype != torch.complex64 or out.device != s.device
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous complex64 {want} tensor on {s.device}")
        out = out.view(F, per)
    lib = _capi.lib()
    _capi.check(lib.lora_mod_batch(int(sf), osr, int(bw), float(amplitude), int(sync) & 0xFF,
                                   s.data_ptr() if S > 0 else None, F, S, out.data_ptr(),
                                   s.device.index, _stream_handle(s.device)))
    return out[0] if squeeze else out


_PREAMBLE_TABLES = {}


def preamble_tables(sf: int, osr: int = 1, bw: int = 125000, amplitude: float = 1.0, preamble: int = 8,
                    device=None):
    """The two fixed parts of a preambled frame (include/lora_mi355x.h, "Preambled frames") as
    complex64 device tensors: ``(pre, sfd)`` - ``preamble`` up-chirps (``preamble * step``
    samples) and the start-of-frame delimiter, two down-chirps and a quarter (``9 * step // 4``).
    Computed once per configuration on the host (lora_preamble_tables) and kept on the device."""
    osr = int(osr) if osr else 1
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise TypeError("preamble_tables lives on a CUDA (HIP) device; there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (int(sf), osr, int(bw), float(amplitude), int(preamble), dev.index)
    if key not in _PREAMBLE_TABLES:
        lib = _capi.lib()
        n = _capi.check(lib.lora_preamble_tables(int(sf), osr, int(bw), float(amplitude), int(preamble), None, None))
        step = n // int(preamble)
        pre = torch.empty(n, dtype=torch.complex64)
        sfd = torch.empty(9 * step // 4, dtype=torch.complex64)
        _capi.check(lib.lora_preamble_tables(int(sf), osr, int(bw), float(amplitude), int(preamble), pre.data_ptr(),
                                             sfd.data_ptr()))
        _PREAMBLE_TABLES[key] = (pre.to(dev), sfd.to(dev))
    return _PREAMBLE_TABLES[key]


def _with_preamble(iq: torch.Tensor, step: int, pre: torch.Tensor, sfd: torch.Tensor) -> torch.Tensor:
    """[pre | iq[.., :2 * step] | sfd | iq[.., 2 * step:]] along the last dimension."""
    lead = iq.shape[:-1]
    return torch.cat([pre.expand(lead + pre.shape), iq[..., :2 * step], sfd.expand(lead + sfd.shape),
                      iq[..., 2 * step:]], dim=-1)


def modulate_preamble(symbols: torch.Tensor, sf: int, osr: int = 1, bw: int = 125000, amplitude: float = 1.0,
                      sync: int = 0x12, preamble: int = 8) -> torch.Tensor:
    """``modulate`` with a preamble and a start-of-frame delimiter: per frame ``preamble`` up-chirps,
    the two sync symbols, two and a quarter down-chirps, the data symbols - ``(preamble + 2 + S) *
    step + 9 * step // 4`` samples.  The sync and data parts are ``modulate``'s frame bit for bit;
    the phase is not continuous across the three joins (include/lora_mi355x.h says why).
    ``modulate`` and one ``torch.cat``: transmit is not the hot path."""
    iq = modulate(symbols, sf, osr, bw, amplitude, sync)
    pre, sfd = preamble_tables(sf, osr, bw, amplitude, preamble, iq.device)
    return _with_preamble(iq, (1 << int(sf)) * (int(osr) if osr else 1), pre, sfd)


class LoRaMod:
    """Block-style modulator mirroring the Pothos ``/lora/lora_mod`` surface
    (examples/lora_simulation.pth:312-326: sf, sync, padding, ampl, ovs) plus bw."""

    def __init__(self, sf: int, sync: int = 0x12, padding: int = 0, ampl: float = 1.0,
                 ovs: int = 1, bw: int = 125000, device=None, cr=1):
        self.sf, self.sync, self.padding = int(sf), int(sync) & 0xFF, int(padding)
        self.cr = cr  # coding rate of work_payload(chain="lora"), as codes.rdd_of takes it
        self.ampl, self.ovs, self.bw = float(ampl), int(ovs) if ovs else 1, int(bw)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)

    def work(self, symbols) -> torch.Tensor:
        if not isinstance(symbols, torch.Tensor):
            symbols = torch.as_tensor(symbols, dtype=torch.int32)
        symbols = symbols.to(self.device)
        iq = modulate(symbols, self.sf, self.ovs, self.bw, self.ampl, self.sync)
        if self.padding > 0:  # trailing zero samples between packets (block "padding")
            pad = torch.zeros(iq.shape[:-1] + (self.padding,), dtype=iq.dtype, device=iq.device)
            iq = torch.cat([iq, pad], dim=-1)
        return iq

    def work_wideband(self, synth, symbols, channel, starts, chan_len: int, dtype=None) -> torch.Tensor:
        """``work`` into a wideband stream (``lora_phy_amd.stream.transmit_wideband`` with this
        block's frames): modulate the [K, S] ``symbols``, put frame i at sample ``starts[i]`` (in
        channel samples) of channel ``channel[i]`` of ``synth``, a ``stream.Synthesizer``, among
        ``chan_len`` samples per channel, and synthesize the one wideband stream: [W] complex64,
        or with ``dtype`` ``torch.int16`` / ``int8`` / ``uint8`` the raw [W, 2] samples that
        ``iq_io.write_raw`` writes for a radio.  This block's rate (bw * ovs) is the channel rate:
        the wideband rate is ``synth.interp`` times it.  The padding of ``work`` is part of each
        frame."""
        from . import stream

        frames = self.work(symbols)
        if frames.dim() == 1:
            frames = frames.unsqueeze(0)
        return stream.transmit_wideband(synth, frames, channel, starts, chan_len, dtype=dtype)

    def work_frame(self, payload, nbytes=None, crc: bool = True, preamble: Optional[int] = None) -> torch.Tensor:
        """Self-describing frames (``codec.encode_frame`` at this block's ``sf`` and ``cr``), then
        modulated: ``payload`` is uint8 [F, max_bytes] (or [max_bytes]), of which frame f carries
        ``nbytes[f]`` bytes (an int32 [F] tensor or a sequence; None: max_bytes each).  Every row
        is as long as the longest possible frame; a shorter frame is followed by silence - zero
        samples, not zero symbols - so a receiver sees nothing after its last symbol.  Nothing is
        read back: the frame lengths stay on the device.  (SF 7-12.)  ``preamble`` (4..64): each
        frame as a preambled frame (``modulate_preamble``: that many up-chirps in front, the
        delimiter between the sync symbols and the data), the silence after it as before; ``work``'s
        padding then follows the frame."""
        from . import codec

        if not isinstance(payload, torch.Tensor):
            payload = torch.as_tensor(payload, dtype=torch.uint8)
        payload = payload.to(self.device)
        if nbytes is not None:
            nbytes = torch.as_tensor(nbytes, dtype=torch.int32).to(self.device).reshape(-1)
        symbols, nsym = codec.encode_frame(payload, nbytes, self.sf, self.cr, crc=crc)
        iq = self.work(symbols)
        step = (1 << self.sf) * self.ovs
        live = torch.arange(iq.shape[-1], device=self.device) < ((nsym.to(torch.int64) + 2) * step)[:, None]
        zero = torch.zeros((), dtype=iq.dtype, device=self.device)
        iq = torch.where(live if iq.dim() == 2 else live[0], iq, zero)
        if preamble is None:
            return iq
        return _with_preamble(iq, step, *preamble_tables(self.sf, self.ovs, self.bw, self.ampl, preamble, self.device))

    def work_payload(self, payload, chain: str = "library", append_crc: bool = False) -> torch.Tensor:
        """Encode payload bytes ([F, n] or [n] uint8) on the device (lora_phy_amd.codec), then
        modulate.  ``chain="library"``: lora_encode (LoRaEncoder.cpp:8-19), with
        ``append_crc`` the SX1272 data checksum appended; ``chain="lora"``: the coding chain at
        this block's ``sf`` and ``cr``."""
        from . import codec

        if chain not in ("library", "lora"):
            raise ValueError('chain must be "library" or "lora"')
        if chain == "lora" and append_crc:
            raise ValueError('append_crc belongs to chain="library"')
        if not isinstance(payload, torch.Tensor):
            payload = torch.as_tensor(payload, dtype=torch.uint8)
        payload = payload.to(self.device)
        if chain == "lora":
            symbols = codec.encode_chain(payload, self.sf, self.cr)
        else:
            symbols = codec.encode(payload, append_crc=append_crc)
        return self.work(symbols)
