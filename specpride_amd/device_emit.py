"""Opt-in device-side MGF emit (``SPX_DEVICE_EMIT=1``): the peak lines of the binning
and gap-average CLIs' writers formatted on the GPU (``spx_format_peaks``,
csrc/mgf_format.hip), the counterpart of :mod:`specpride_amd.device_ingest`.
:func:`write_records` takes any list of peak segments in any of the three record
styles; the medoid CLI does not use it yet.

The peaks never cross to the host as doubles: the kernel writes each record's
``repr(mz) repr(inten)`` lines into HBM, the text comes back with ``spx_copy_d2h``
and the host writer (``spx_mgf_splice_records``) formats only the record headers and
splices the blocks in.  The oracle is ``mgf_native.write_records`` over the same
records; the files are byte-identical.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib, engine, mgf_native

ENV = "SPX_DEVICE_EMIT"
STAGES = ("small_readback", "compaction", "format", "text_d2h", "write")


def enabled() -> bool:
    return os.environ.get(ENV) == "1"


def _ptr(a):
    return a.ctypes.data


def splice_records(path, style: int, titles, text_off, text, prec, charge, rt=None, flags=None,
                   append: bool = False, threads: int = 0) -> None:
    """:func:`mgf_native.write_records` with record c's peak lines given as text
    (``text[text_off[c]:text_off[c + 1]]``, host arrays) instead of doubles."""
    C = len(titles)
    if any("\n" in t for t in titles):
        raise ValueError("record titles cannot contain a newline")
    text_off = np.ascontiguousarray(text_off, np.int64)
    text = np.ascontiguousarray(text, np.uint8)
    if len(text_off) != C + 1:
        raise ValueError("text_off must have len(titles) + 1 entries")
    if C and (text_off[0] < 0 or text_off[-1] > len(text) or np.any(np.diff(text_off) < 0)):
        raise ValueError("text offsets out of range")
    prec = np.ascontiguousarray(prec, np.float64)
    charge = np.ascontiguousarray(charge, np.int64)
    rt = np.ascontiguousarray(rt if rt is not None else np.full(C, np.nan), np.float64)
    flags = np.ascontiguousarray(flags if flags is not None else np.full(C, 15), np.int32)
    for a in (prec, charge, rt, flags):
        if len(a) != C:
            raise ValueError("per-record arrays must have len(titles) entries")
    joined = "\n".join(titles).encode("utf-8", errors="surrogateescape")
    rc = _lib.lib().spx_mgf_splice_records(os.fsencode(path), int(bool(append)), int(style), C, joined, _ptr(flags),
                                           _ptr(prec), _ptr(charge), _ptr(rt), _ptr(text_off), _ptr(text),
                                           int(threads))
    if rc != 0:
        raise OSError(f"spx_mgf_splice_records failed writing {path}")


def _device_i64(a, dev):
    import torch

    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.int64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev)


def write_consensus(path, style: int, titles, res, raise_for, append: bool = False, stages=None) -> None:
    """The records of a device result (:class:`engine.PeaksResult` of bin-mean or
    gap-average): only the per-cluster arrays are read back (``small_readback``),
    ``raise_for(status)`` raises the CLI's error for the first failing cluster before
    anything is written, then the peaks are compacted (``compaction``) and written by
    :func:`write_records` without leaving the device as doubles."""
    import torch

    from .device_ingest import _Clock

    batch = res.batch
    C, dev = batch.n_clusters, batch.device
    clock = _Clock(stages, dev)
    with torch.cuda.device(dev):
        if res.stream is not None:
            torch.cuda.current_stream(dev).wait_stream(res.stream)
        items = [("count", res.count[:C]), ("status", res.status[:C]), ("prec", res.prec[:C]),
                 ("charge", res.charge[:C])]
        if res.rt is not None:
            items.append(("rt", res.rt[:C]))
        h = engine._packed_to_host(items)
    clock.lap("small_readback")
    bad = np.flatnonzero(h["status"] != engine.STATUS_OK)
    if len(bad):
        raise_for(int(h["status"][bad[0]]))
    out_off, dmz, dint = res.compact(total=int(h["count"].sum()))
    clock.lap("compaction")
    write_records(path, style, titles, dmz, dint, out_off[:-1], out_off[1:], h["prec"], h["charge"].astype(np.int64),
                  h.get("rt"), None, append, batch=batch, stages=stages)


def write_records(path, style: int, titles, mz, inten, seg_begin, seg_end, prec, charge, rt=None, flags=None,
                  append: bool = False, batch=None, stages=None) -> None:
    """Write len(titles) MGF records whose peaks are in HBM: record c's peaks are
    ``mz/inten[seg_begin[c]:seg_end[c]]`` (device tensors; the segments device
    tensors or host arrays), the per-record fields host arrays as for
    :func:`mgf_native.write_records`.  Style 0 skips peaks with a NaN intensity, as
    the host writer does.  Nothing is written unless the whole text was formatted:
    a set flag bit (capacity, a bad segment range) raises first.  ``stages`` (a
    dict) receives the seconds per stage of :data:`STAGES`, each ending in a
    device synchronisation."""
    from .device_ingest import _Clock

    dev = mz.device
    clock = _Clock(stages, dev)
    fr = engine.format_peaks(mz, inten, _device_i64(seg_begin, dev), _device_i64(seg_end, dev),
                             skip_nan=style == mgf_native.STYLE_BINNING, batch=batch)
    clock.lap("format")
    h = fr.to_host()
    clock.lap("text_d2h")
    if h["flags"]:
        raise RuntimeError(f"spx_format_peaks reported flags {h['flags']} (1: text capacity, 2: segment range); "
                           f"{path} not written")
    splice_records(path, style, titles, h["text_off"], h["text"], prec, charge, rt, flags, append)
    clock.lap("write")
