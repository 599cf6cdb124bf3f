"""Drop-in for the reference's evaluation module ``src/benchmark.py`` (binned
cosine, benchmark.py:7-38, and explained b/y intensity, :40-61) on the MI355X
engine (``spx_binned_cosine``, ``spx_cosine_medoid``, ``spx_by_fraction``).

Same names and argument meanings as the reference: spectra are objects with
``.mz`` and ``.intensity`` arrays (spectrum_utils ``MsmsSpectrum`` or anything
alike).  ``cos_dist`` / ``average_cos_dist`` evaluate one representative;
``average_cos_dist_batch`` evaluates every cluster of a file in one device pass;
``most_similar_by_cosine`` picks each cluster's most similar member (``spx_cosine_medoid``).
An empty spectrum raises IndexError, as the reference's ``mz[-1]`` does.
``fraction_of_by`` scores one spectrum against its peptide, ``fraction_of_by_batch``
any number of them in one device call, ``best_by_explained`` picks each cluster's
member with the highest fraction; ``python -m specpride_amd.benchmark IN.mgf``
prints the fraction of every spectrum of a clustered MGF.
"""
from __future__ import annotations

import sys

import numpy as np

from . import engine
from .csr import SpectraCSR

mz_unit = 1.000508         # benchmark.py:7
mz_space = mz_unit * .005  # benchmark.py:8


def _arrays(spec):
    return np.asarray(spec.mz, np.float64), np.asarray(spec.intensity, np.float64)


def average_cos_dist_batch(representatives, clusters, mz_space=mz_space, device="cuda"):
    """[average_cos_dist(representatives[c], clusters[c]) for every c] and the
    per-member cosines, from ONE engine call.  Returns (avg [C], cos: list of
    per-cluster arrays)."""
    import torch

    csr = SpectraCSR.from_clusters([[{"m/z array": _arrays(s)[0], "intensity array": _arrays(s)[1]} for s in cl]
                                    for cl in clusters])
    reps = [_arrays(r) for r in representatives]
    if len(reps) != csr.n_clusters:
        raise ValueError("one representative per cluster")
    rep_off = np.zeros(len(reps) + 1, np.int64)
    np.cumsum([len(m) for m, _ in reps], out=rep_off[1:])
    rep_mz = np.concatenate([m for m, _ in reps]) if reps else np.zeros(0)
    rep_int = np.concatenate([i for _, i in reps]) if reps else np.zeros(0)
    batch = engine.DeviceBatch.from_host(csr, device=device)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    t_off, t_mz, t_int = dev(rep_off), dev(rep_mz if len(rep_mz) else np.zeros(1)), dev(
        rep_int if len(rep_int) else np.zeros(1))
    cos, avg, status = engine.binned_cosine(batch, t_off, t_mz, t_int, mz_space=mz_space).to_host()
    for c, st in enumerate(status[:csr.n_clusters]):
        if st == engine.STATUS_EMPTY:
            raise IndexError("index -1 is out of bounds for axis 0 with size 0")  # benchmark.py:20 mz[-1]
        if st != engine.STATUS_OK:
            raise RuntimeError(f"cluster {c}: binned cosine unresolved (status {st})")
    return avg[:csr.n_clusters], [cos[csr.cluster_off[c]:csr.cluster_off[c + 1]] for c in range(csr.n_clusters)]


def most_similar_by_cosine(clusters, mz_space=mz_space, device="cuda"):
    """For every cluster (a list of spectrum objects) the index of the member with the
    highest ``average_cos_dist(member, cluster)`` -- the first one among equals -- and
    every member's average, from ONE engine call.  Returns (indices: list of int, -1 for
    an empty cluster; scores: list of per-cluster arrays)."""
    csr = SpectraCSR.from_clusters([[{"m/z array": _arrays(s)[0], "intensity array": _arrays(s)[1]} for s in cl]
                                    for cl in clusters])
    batch = engine.DeviceBatch.from_host(csr, device=device)
    rep, score, status = engine.cosine_medoid(batch, mz_space=mz_space, with_scores=True).to_host()
    indices = []
    for c, st in enumerate(status[:csr.n_clusters]):
        if st == engine.STATUS_EMPTY:
            raise IndexError("index -1 is out of bounds for axis 0 with size 0")  # benchmark.py:20 mz[-1]
        if st != engine.STATUS_OK:
            raise RuntimeError(f"cluster {c}: cosine medoid unresolved (status {st})")
        indices.append(int(rep[c] - csr.cluster_off[c]) if rep[c] >= 0 else -1)
    return indices, [score[csr.cluster_off[c]:csr.cluster_off[c + 1]] for c in range(csr.n_clusters)]


def cos_dist(representative_spectrum, cluster_member):
    """benchmark.py:19-29: binned cosine of a representative and one member."""
    _, cos = average_cos_dist_batch([representative_spectrum], [[cluster_member]])
    return float(cos[0][0])


def average_cos_dist(representative_spectrum, cluster_members):
    """benchmark.py:31-38: mean cosine of the representative to the members (0.0 if none)."""
    avg, _ = average_cos_dist_batch([representative_spectrum], [list(cluster_members)])
    return float(avg[0])


VALID_RESIDUES = frozenset("QWERTYIPASDFGHKLCVNM")  # pyteomics parser.std_amino_acids


def fast_valid(peptide_seq) -> bool:
    """pyteomics ``parser.fast_valid``: every character is one of the 20 standard residues."""
    return set(peptide_seq) <= VALID_RESIDUES


def peptide_of_title(title: str) -> str:
    """The peptide of a clustered MGF's title ``...:scan:N:PEPTIDE/z`` (benchmark.py:68)."""
    return title.split(':')[-1][:-2]


def title_has_peptide(title: str) -> bool:
    """The title's last ':' field ends in ``/z`` behind at least one character."""
    last = title.split(':')[-1]
    return len(last) >= 3 and last[-2] == '/'


def _by_device(peptides, precursor_mzs, precursor_charges, arrays, device):
    """The inputs of ``engine.by_fraction`` on ``device`` for spectra given as (mz, intensity)
    arrays; an invalid peptide (or None: there is none) is reported on stderr (benchmark.py:42)
    and sent as one byte that is no residue (the kernel gives it 0.0)."""
    import torch

    n = len(arrays)
    if not (len(peptides) == len(precursor_mzs) == len(precursor_charges) == n):
        raise ValueError("one peptide, precursor m/z and charge per spectrum")
    valid = np.ones(n, bool)
    seqs = []
    for k, pep in enumerate(peptides):
        if pep is None or not fast_valid(pep):
            print("Invalid peptide sequence encountered", file=sys.stderr)
            valid[k] = False
            pep = "?"  # one byte that is no residue, whatever the string held
        seqs.append(pep.encode("ascii"))
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(m) for m, _ in arrays], out=off[1:])
    seq_off = np.zeros(n + 1, np.int64)
    np.cumsum([len(b) for b in seqs], out=seq_off[1:])
    for m, i in arrays:
        if len(m) != len(i):
            raise ValueError("m/z and intensity arrays differ in length")
    mz = np.concatenate([m for m, _ in arrays]) if n else np.zeros(0)
    inten = np.concatenate([i for _, i in arrays]) if n else np.zeros(0)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    t_off = dev(off)
    args = (dev(mz), dev(inten), t_off[:-1].contiguous(), t_off[1:].contiguous(),
            dev(np.asarray(precursor_mzs, np.float64)), dev(np.asarray(precursor_charges, np.int32)),
            dev(np.frombuffer(b"".join(seqs), np.uint8).copy()), dev(seq_off))
    return args, valid


def _by_checked(fraction, status, valid):
    """Host fractions after the statuses: an invalid peptide is 0.0 whatever its spectrum."""
    fraction = np.where(valid, fraction[:len(valid)], 0.0)
    for k in np.flatnonzero(valid & (status[:len(valid)] != engine.STATUS_OK)):
        raise ValueError(f"spectrum {k}: explained b/y intensity unresolved (a non-finite m/z or precursor m/z, "
                         f"more than {engine.BY_MAX_SEQ} residues or a charge above {engine.BY_MAX_CHARGE})")
    return fraction


def fraction_of_by_batch(peptides, precursor_mzs, precursor_charges, spectra, device="cuda"):
    """[fraction_of_by(peptides[k], precursor_mzs[k], precursor_charges[k], spectra[k].mz,
    spectra[k].intensity) for every k] from ONE engine call.  Returns a float64 array."""
    args, valid = _by_device(peptides, precursor_mzs, precursor_charges, [_arrays(s) for s in spectra], device)
    fraction, status = engine.by_fraction(*args).to_host()
    return _by_checked(fraction, status, valid)


def fraction_of_by(peptide_seq, precursor_mz, precursor_charge, mz, intensity, device="cuda"):
    """benchmark.py:40-61: the share of the spectrum's intensity (100 <= m/z <= 1400, precursor
    peaks removed) that the b/y ions of ``peptide_seq`` annotate at 50 ppm."""
    args, valid = _by_device([peptide_seq], [precursor_mz], [precursor_charge],
                             [(np.asarray(mz, np.float64), np.asarray(intensity, np.float64))], device)
    fraction, status = engine.by_fraction(*args).to_host()
    return float(_by_checked(fraction, status, valid)[0])


def best_by_explained(clusters, peptides, device="cuda"):
    """For every cluster (a list of spectrum objects with ``.mz``, ``.intensity``,
    ``.precursor_mz`` and ``.precursor_charge``) the index of the first member with the
    highest ``fraction_of_by`` against the cluster's peptide, -1 for an empty cluster:
    ``engine.by_fraction`` then ``engine.best_score`` with rank = member ordinal.  Returns
    (indices: list of int, fractions: list of per-cluster arrays)."""
    import torch

    if len(peptides) != len(clusters):
        raise ValueError("one peptide per cluster")
    members = [s for cl in clusters for s in cl]
    cluster_off = np.zeros(len(clusters) + 1, np.int64)
    np.cumsum([len(cl) for cl in clusters], out=cluster_off[1:])
    args, valid = _by_device([p for p, cl in zip(peptides, clusters) for _ in cl],
                             [s.precursor_mz for s in members], [s.precursor_charge for s in members],
                             [_arrays(s) for s in members], device)
    got = engine.by_fraction(*args)
    n = len(members)
    t_off = torch.as_tensor(cluster_off, device=device)
    best, _ = engine.best_score(t_off, got.fraction[:n], torch.arange(n, dtype=torch.int64, device=device)).to_host()
    fraction, status = got.to_host()
    fraction = _by_checked(fraction, status, valid)
    # an invalid peptide's members all score 0.0 on the device as well: the first one wins
    indices = [int(best[c] - cluster_off[c]) if cluster_off[c + 1] > cluster_off[c] else -1
               for c in range(len(clusters))]
    return indices, [fraction[cluster_off[c]:cluster_off[c + 1]] for c in range(len(clusters))]


def main(argv=None, device="cuda") -> int:
    """``python -m specpride_amd.benchmark IN.mgf``: one line ``<title>\t<repr(fraction)>`` per
    spectrum of a clustered MGF (titles ``...:PEPTIDE/z``, as convert_mgf_cluster writes
    them), every fraction from one device call."""
    from .mgf import read_mgf

    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        print("usage: python -m specpride_amd.benchmark IN.mgf", file=sys.stderr)
        return 2
    spectra = read_mgf(argv[0])
    titles = [sp["params"].get("title", "") for sp in spectra]
    # a title with no peptide part is an invalid peptide: 0.0 and the message
    args, valid = _by_device([peptide_of_title(t) if title_has_peptide(t) else None for t in titles],
                             [sp["params"]["pepmass"][0] for sp in spectra],
                             [sp["params"]["charge"][0] for sp in spectra],
                             [(sp["m/z array"], sp["intensity array"]) for sp in spectra], device)
    fraction, status = engine.by_fraction(*args).to_host()
    for title, f in zip(titles, _by_checked(fraction, status, valid)):
        print(f"{title}\t{float(f)!r}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
