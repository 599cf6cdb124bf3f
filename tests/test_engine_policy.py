"""The engine's medoid state rules (engine.medoid_mode / medoid_learn / medoid_resolve /
fused_stage) on a plain dict and hand-written ``rep`` codes: what a batch remembers
after a checked call, and what the calls after it do with it.  No device, no library."""
import numpy as np

from specpride_amd import _lib, engine
from specpride_amd.engine import REP_ARENA, REP_DEFERRED, REP_EMPTY, REP_RANGE


def _rep(n=10, **codes):
    """n resolved clusters (rep = own index), with ``c<k>=code`` overrides."""
    rep = np.arange(n, dtype=np.int64)
    for k, code in codes.items():
        rep[int(k[1:])] = code
    return rep


def _size_key(ws, tol):
    return ("medoid_size", engine.medoid_mode(ws, False, tol)[1])


def test_no_codes_no_rerun_nothing_stored():
    ws = {}
    assert not engine.medoid_unresolved(_rep())
    assert engine.medoid_learn(ws, 0.1, _rep()) is False
    # final codes are not a reason to re-run either
    assert engine.medoid_learn(ws, 0.1, _rep(c3=REP_EMPTY, c4=REP_RANGE)) is False
    assert ws == {}
    assert engine.medoid_mode(ws, False, 0.1) == (False, ())
    assert engine.medoid_mode(ws, True, 0.1) == (True, ())


def test_deferred_keeps_large_path_on_at_that_tolerance_only():
    """The defect fixed in e914d3e: the unchecked calls after a checked one that met a
    run-time deferral must keep the large path on, at the tolerance it was seen at."""
    ws = {}
    assert engine.medoid_learn(ws, 0.1, _rep(c6=REP_DEFERRED)) is True
    for _ in range(3):  # every later call
        assert engine.medoid_mode(ws, False, 0.1) == (True, ())
    assert engine.medoid_mode(ws, False, 0.02) == (False, ())  # not large by size: off elsewhere
    assert engine.medoid_mode(ws, True, 0.02) == (True, ())
    assert ws.get("medoid_extra") == ()  # nothing ran out of arena


def test_arena_clusters_accumulate_sorted_and_change_the_size_key():
    ws = {}
    key0 = _size_key(ws, 0.1)
    assert engine.medoid_learn(ws, 0.1, _rep(c7=REP_ARENA, c2=REP_ARENA)) is True
    assert ws["medoid_extra"] == (2, 7)
    key1 = _size_key(ws, 0.1)
    assert engine.medoid_learn(ws, 0.1, _rep(c2=REP_ARENA, c5=REP_ARENA)) is True
    assert ws.get("medoid_extra") == (2, 5, 7)
    assert all(isinstance(c, int) for c in ws["medoid_extra"])
    key2 = _size_key(ws, 0.1)
    assert len({key0, key1, key2}) == 3 and key2 == ("medoid_size", (2, 5, 7))
    for tol in (0.1, 0.02, 0.5):  # budgeted clusters need the large path at every tolerance
        assert engine.medoid_mode(ws, False, tol) == (True, (2, 5, 7))


def _fused_key(ws, tol):
    prm = _lib.SpxBinParams(100.0, 2000.0, 0.02, 1)
    return engine.fused_key(prm, _lib.SpxMedoidParams(tol, int(engine.medoid_mode(ws, False, tol)[0])))


def test_fused_clean_flag_is_forgotten_when_a_deferral_is_learned():
    ws = {}
    key = _fused_key(ws, 0.1)
    assert key[0] == "fused_clean" and key[-1] == 0
    assert engine.fused_stage(ws, key) == 0  # nothing remembered: the whole pass
    assert engine.fused_stage(ws, key, clean=False) == 0 and ws[key] is False
    assert engine.fused_stage(ws, key, clean=True) == 1 and ws[key] is True
    assert engine.fused_stage(ws, _fused_key(ws, 0.1)) == 1  # later unchecked calls: stage 1 alone
    assert engine.medoid_learn(ws, 0.1, _rep(c1=REP_DEFERRED)) is True
    late = _fused_key(ws, 0.1)
    assert late != key and late[-1] == 1
    assert engine.fused_stage(ws, late) == 0  # the remembered "clean" is not found
    assert engine.fused_stage(ws, _fused_key(ws, 0.02)) == 0  # and was never set at 0.02


def test_resolve_stops_when_clean_and_after_two_reruns():
    launches = []

    def codes_after(n_bad_rounds):
        reads = iter([_rep(c4=REP_ARENA)] * n_bad_rounds + [_rep()] * 3)
        return lambda: next(reads)

    ws = {}
    engine.medoid_resolve(ws, 0.1, codes_after(0), lambda: launches.append(dict(ws)))
    assert launches == [] and ws == {}
    engine.medoid_resolve(ws, 0.1, codes_after(1), lambda: launches.append(dict(ws)))
    assert len(launches) == 1  # one re-run, launched after the batch learned
    assert launches[0]["medoid_extra"] == (4,) and launches[0][("medoid_late", 0.1)] is True

    launches.clear()
    reads = []

    def always_bad():
        reads.append(1)
        return _rep(c4=REP_ARENA)

    engine.medoid_resolve({}, 0.1, always_bad, lambda: launches.append(1))
    assert len(reads) == 2 and len(launches) == 2  # the codes persist: it gives up after two
