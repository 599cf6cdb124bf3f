"""Opt-in device-side MGF ingest (``SPX_DEVICE_INGEST=1``): the number parsing of
the three CLIs' readers moved to the GPU (``spx_parse_mgf_text``, csrc/mgf_parse.hip).

The host indexes the file (``mgf_native.index``: byte range, title and peak-line
count per record, no number parsed) and groups the titles the CLI's way
(:mod:`specpride_amd.ingest`); the raw bytes go to HBM with ``spx_copy_h2d`` and
one kernel writes the cluster-segmented CSR directly in cluster order -- no host
CSR, no permutation copy, no second H2D.

The oracle is the host parser ``mgf_native.parse_ranges`` over the same records in
the same order.  The kernel reports ``OK`` or ``REPARSE`` per record; a record it
cannot decide with certainty is re-parsed on the host and patched into the device
arrays, so the result is bit-identical to the host's -- or the whole file is
outside the native subset ("fallback:") and :func:`load` returns None: the caller
then takes the path it takes without the switch.
"""
from __future__ import annotations

import os
import re
import time

import numpy as np

from . import _lib, engine, ingest, mgf_native
from .csr import concat_ranges

ENV = "SPX_DEVICE_INGEST"
OK, REPARSE = 0, 1  # spx_mgf_status
STAGES = ("index", "grouping", "h2d", "kernels", "status_readback", "patching", "batch")

_GROUPS = {mgf_native.GROUP_BINNING: ingest.binning_groups, mgf_native.GROUP_RUNS: ingest.gap_average_groups,
           mgf_native.GROUP_FIRST_RUNS: ingest.medoid_groups}
_PREAMBLE_MAX = 1 << 20


def enabled() -> bool:
    return os.environ.get(ENV) == "1"


class Meta(dict):
    """What the writers need besides the device arrays: ``ids`` (cluster ids),
    ``sizes`` (members per cluster), ``records`` (file record of every CSR spectrum),
    ``has_prec`` / ``has_charge`` / ``has_rt`` / ``has_title`` and ``flags`` per CSR
    spectrum, ``n_reparse``; ``meta["titles"]`` (titles in CSR order) is built on
    first use and :meth:`title` gives one."""

    def __missing__(self, key):
        if key != "titles":
            raise KeyError(key)
        t = self["_index_titles"]
        v = [t[r] for r in self["records"]]
        self["titles"] = v
        return v

    def title(self, s: int) -> str:
        return self["_index_titles"][self["records"][s]]


def plan(titles, npk, group_mode):
    """Destination order of an index: ``(ids, sizes, order, n_used, spec_off)``.
    ``order[:n_used]`` are the records in CSR order (cluster-major, the grouping's
    own), ``order[n_used:]`` the records no cluster takes (the medoid CLI's later
    runs: parsed like the host does, never part of the CSR); ``spec_off`` [R + 1] is
    the prefix sum of the index's peak counts in that order."""
    ids, records, sizes = _GROUPS[group_mode](titles)
    records = np.asarray(records, np.int64)
    n_used = len(records)
    order = records
    if n_used < len(titles):
        taken = np.zeros(len(titles), bool)
        taken[records] = True
        order = np.concatenate([records, np.flatnonzero(~taken)])
    spec_off = np.zeros(len(order) + 1, np.int64)
    np.cumsum(np.asarray(npk, np.int64)[order], out=spec_off[1:])
    return ids, np.asarray(sizes, np.int64), order, n_used, spec_off


def _h2d(a, dev, stream):
    import torch

    a = np.ascontiguousarray(a)
    t = torch.empty(a.shape, dtype=engine.dtype_of(a.dtype), device=dev)
    _lib.check(_lib.lib().spx_copy_h2d(t.data_ptr(), a.ctypes.data, a.nbytes, stream.cuda_stream), "spx_copy_h2d")
    return t


class _Clock:
    """Stage times of one load (seconds); with ``sync`` every stage waits for the
    device, so a stage's time is its own."""

    def __init__(self, stages, dev=None):
        self.stages, self.dev, self.t = stages, dev, time.perf_counter()

    def lap(self, name):
        if self.stages is None:
            return
        if self.dev is not None:
            import torch

            torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        self.stages[name] = self.stages.get(name, 0.0) + (now - self.t)
        self.t = now


def parse_records(path, begin, end, npk, general: bool, device="cuda", title_of=None, stages=None,
                  patch: bool = True):
    """Records [begin[r], end[r]) of ``path`` (byte ranges and peak-line counts of
    ``mgf_native.index``, any order) parsed on the device.  Returns a dict of device
    tensors ``spec_off`` [R+1], ``mz``, ``inten`` [P], ``prec_mz``, ``rt`` [R],
    ``charge`` [R] (int32) plus host arrays ``host_spec_off``, ``flags`` [R] (bit0
    PEPMASS, bit1 CHARGE, general also bit2 RTINSECONDS, bit3 TITLE) and ``status``
    [R] (the kernel's OK / REPARSE); flagged records were re-parsed with
    ``mgf_native.parse_ranges`` and patched in, so every array equals parse_ranges
    over the same records in the same order.  None: the host parser reports the
    records as outside the native subset ("fallback:"), or disagrees with the index
    (``title_of(r)``, if given, is the index's title of record r).  ``patch=False``
    returns the kernel's own output: flagged records are left undefined."""
    import torch

    L = _lib.lib()
    begin = np.ascontiguousarray(begin, np.int64)
    end = np.ascontiguousarray(end, np.int64)
    npk = np.ascontiguousarray(npk, np.int64)
    R = len(begin)
    if len(end) != R or len(npk) != R or (R and npk.min() < 0):
        raise ValueError("begin, end and npk must have one entry per record (npk >= 0)")
    spec_off = np.zeros(R + 1, np.int64)
    np.cumsum(npk, out=spec_off[1:])
    P = int(spec_off[-1])
    size = os.path.getsize(path)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("device ingest needs a HIP device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        clock = _Clock(stages, dev)
        stream = torch.cuda.current_stream(dev)
        text = torch.empty(max(size, 1), dtype=torch.uint8, device=dev)
        if size:
            mm = np.memmap(path, dtype=np.uint8, mode="r")
            _lib.check(L.spx_copy_h2d(text.data_ptr(), mm.ctypes.data, size, stream.cuda_stream), "spx_copy_h2d")
            tail_open = int(mm[size - 1]) not in (10, 13)
            del mm
        else:
            tail_open = False
        d_begin, d_end, d_off = _h2d(begin, dev, stream), _h2d(end, dev, stream), _h2d(spec_off, dev, stream)
        clock.lap("h2d")
        mz = torch.empty(max(P, 1), dtype=torch.float64, device=dev)
        inten = torch.empty(max(P, 1), dtype=torch.float64, device=dev)
        prec = torch.empty(max(R, 1), dtype=torch.float64, device=dev)
        rt = torch.empty(max(R, 1), dtype=torch.float64, device=dev)
        charge = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
        flags = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
        status = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
        _lib.check(L.spx_parse_mgf_text(text.data_ptr(), size, d_begin.data_ptr(), d_end.data_ptr(), d_off.data_ptr(),
                                        R, P, int(bool(general)), mz.data_ptr(), inten.data_ptr(), prec.data_ptr(),
                                        charge.data_ptr(), rt.data_ptr(), flags.data_ptr(), status.data_ptr(),
                                        stream.cuda_stream or None), "spx_parse_mgf_text")
        clock.lap("kernels")
        packed = torch.stack([status[:R], flags[:R]]).cpu().numpy() if R else np.zeros((2, 0), np.int32)
        h_status, h_flags = packed[0].copy(), packed[1].copy()
        del text, d_begin, d_end  # the text buffer is freed here
        clock.lap("status_readback")
        # A last record without a line terminator that is not parsed last: the host
        # parser reads the records as one text, so its last line runs into the next
        # record's first.  The host decides all of it.
        at_eof = np.flatnonzero(end == size)
        if tail_open and len(at_eof) and (len(at_eof) > 1 or at_eof[0] != R - 1):
            h_status[:] = REPARSE
        bad = np.flatnonzero(h_status != OK) if patch else ()
        if len(bad):
            try:
                flat = mgf_native.parse_ranges(path, begin[bad], end[bad], general)
            except ValueError:
                return None
            if not np.array_equal(np.diff(flat["spec_off"]), npk[bad]):
                return None  # the index and the parser disagree on a record's peaks
            if title_of is not None and flat["titles"] != [title_of(int(r)) for r in bad]:
                return None
            if len(flat["charge"]) and np.abs(flat["charge"]).max() > np.iinfo(np.int32).max:
                return None
            f = flat["has_prec"].astype(np.int32) | (flat["has_charge"].astype(np.int32) << 1)
            if general:
                f |= (flat["has_rt"].astype(np.int32) << 2) | (flat["has_title"].astype(np.int32) << 3)
            h_flags[bad] = f
            d_bad = _h2d(bad, dev, stream)
            dst = _h2d(concat_ranges(spec_off[bad], npk[bad]), dev, stream)
            mz.index_copy_(0, dst, _h2d(flat["mz"], dev, stream))
            inten.index_copy_(0, dst, _h2d(flat["inten"], dev, stream))
            prec.index_copy_(0, d_bad, _h2d(flat["prec_mz"], dev, stream))
            charge.index_copy_(0, d_bad, _h2d(flat["charge"].astype(np.int32), dev, stream))
            rt.index_copy_(0, d_bad, _h2d(flat["rt"] if general else np.full(len(bad), np.nan), dev, stream))
        clock.lap("patching")
    return dict(spec_off=d_off, mz=mz[:P], inten=inten[:P], prec_mz=prec[:R], rt=rt[:R], charge=charge[:R],
                host_spec_off=spec_off, flags=h_flags, status=h_status)


def _preamble_ok(path, first_begin: int, general: bool) -> bool:
    """The bytes before the first indexed record, as the whole-file host parsers see
    them: only lines they pass over (blank; for the binning reader also BEGIN IONS;
    for the general reader any ASCII line but END IONS)."""
    if first_begin == 0:
        return True
    if first_begin > _PREAMBLE_MAX:
        return False
    with open(path, "rb") as fh:
        pre = fh.read(first_begin)
    if any(b == 0 or b >= 0x80 for b in pre):
        return False
    lines = [ln.strip() for ln in re.split("\r\n|\n|\r", pre.decode("ascii"))]
    if general:
        return all(ln != "END IONS" for ln in lines)
    return all(ln in ("", "BEGIN IONS") for ln in lines)


def load(path, general: bool, group_mode: int, device="cuda", stages=None):
    """``(DeviceBatch, Meta)`` of an MGF file grouped the CLI's way (``group_mode``:
    ``mgf_native.GROUP_*``), parsed on the device, or None when the file as a whole
    is outside the native subset (or the native libraries' index is unavailable):
    the caller then takes the path it takes without the switch.  ``stages`` (a
    dict) receives the seconds per stage of :data:`STAGES`."""
    import torch

    clock = _Clock(stages)
    try:
        X = mgf_native.index(path, general)
    except ValueError:
        return None
    clock.lap("index")
    if X is None or len(X["begin"]) == 0:
        return None
    titles = X["titles"]
    # whole-file checks of the host paths that live outside the records
    if not general and not all(";" in t for t in titles):  # the reference's parts[1] raises
        return None
    if not _preamble_ok(path, int(X["begin"].min()), general):
        return None
    ids, sizes, order, n_used, _off = plan(titles, X["npk"], group_mode)
    clock.lap("grouping")
    got = parse_records(path, X["begin"][order], X["end"][order], X["npk"][order], general, device,
                        title_of=lambda r: titles[order[r]], stages=stages)
    if got is None:
        return None
    flags = got["flags"]
    need = 8 if general else 3  # every record: a TITLE (general), PEPMASS and CHARGE (binning)
    if not np.all((flags & need) == need):
        return None
    clock = _Clock(stages, got["mz"].device)
    host_spec_off = got["host_spec_off"][:n_used + 1]
    n_peaks = int(host_spec_off[-1])
    cluster_off = ingest.cluster_starts(sizes)
    dev = got["mz"].device
    with torch.cuda.device(dev):
        tensors = dict(cluster_off=torch.from_numpy(cluster_off).to(dev), spec_off=got["spec_off"][:n_used + 1],
                       mz=got["mz"][:n_peaks], inten=got["inten"][:n_peaks], prec_mz=got["prec_mz"][:n_used],
                       charge=got["charge"][:n_used], rt=got["rt"][:n_used], n_clusters=len(sizes),
                       n_spectra=n_used, n_peaks=n_peaks)
        batch = engine.DeviceBatch(tensors, cluster_off, host_spec_off, engine.device_span(tensors["mz"]),
                                   cluster_ids=ids)
    f = flags[:n_used]
    meta = Meta(ids=ids, sizes=sizes, records=order[:n_used], flags=f, has_prec=(f & 1) != 0,
                has_charge=(f & 2) != 0, has_rt=(f & 4) != 0, has_title=(f & 8) != 0,
                n_reparse=int(np.count_nonzero(got["status"] != OK)), n_records=len(order), _index_titles=titles)
    clock.lap("batch")
    return batch, meta


def chosen_records(batch, meta, chosen):
    """Host copies of the CSR spectra ``chosen`` (the medoid CLI's writer input):
    ``(titles, off, mz, inten, prec, charge, rt, flags)`` gathered on the device."""
    import torch

    chosen = np.asarray(chosen, np.int64)
    so = batch.host_spec_off
    lens = so[chosen + 1] - so[chosen]
    off = ingest.cluster_starts(lens)
    dev = batch.device
    idx = torch.from_numpy(concat_ranges(so[chosen], lens)).to(dev)
    ct = torch.from_numpy(chosen).to(dev)
    return ([meta.title(int(s)) for s in chosen], off, batch.t["mz"][idx].cpu().numpy(),
            batch.t["inten"][idx].cpu().numpy(), batch.t["prec_mz"][ct].cpu().numpy(),
            batch.t["charge"][ct].cpu().numpy().astype(np.int64), batch.t["rt"][ct].cpu().numpy(),
            meta["flags"][chosen].astype(np.int32))
