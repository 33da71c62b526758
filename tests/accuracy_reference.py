"""Lattice/Accuracy.cc restated in plain Python and numpy.float32, with the reference's own containers: per frame of the reference lattice
a dict token -> set of (start, end) (ActiveStates, :523-553; the reference keys the sets by the run's first label and compares label() of
it, which is the token), a fresh dict per run of the hypothesis (:622-633).  Checked by reading against the cited lines; there is no
golden file.  A key is (segment, tbeg, tokens), tokens None where the aligner reached no final state."""
import numpy as np

from tests.quanteq_reference import mad32

F32 = np.float32


def runs(tbeg, tokens):
    """maximal stretches of one token (:614-620): [(token, start, end)]"""
    out, i = [], 0
    while tokens is not None and i < len(tokens):
        j = i
        while j < len(tokens) and tokens[j] == tokens[i]:
            j += 1
        out.append((int(tokens[i]), tbeg + i, tbeg + j))
        i = j
    return out


def active_states(ref_keys, per_frame=False):
    """discoverState (:523-553; per_frame: FrameStateAccuracyAutomaton's, :822-840) over one segment's reference keys"""
    frames = {}
    for _, tbeg, tokens in ref_keys:
        for tok, s, e in ([(int(t), tbeg + i, tbeg + i + 1) for i, t in enumerate(tokens or [])] if per_frame else runs(tbeg, tokens)):
            for t in range(s, e):
                frames.setdefault(t, {}).setdefault(tok, set()).add((s, e))
    return frames


def table(frames):
    """what amx_accuracy_last_reference returns: rows (token, start, end), ascending in (start, end, token)"""
    rows = sorted({(s, e, tok) for states in frames.values() for tok, ivs in states.items() for s, e in ivs})
    return np.array([(tok, s, e) for s, e, tok in rows], np.int32).reshape(-1, 3)


def approximate(refs, tok, hs, he):
    """ApproximateAccuracyAutomaton::accuracy (:361-380)"""
    if not refs:
        return F32(0)
    acc = F32(-3.40282347e+38)
    for rtok, ivs in refs.items():
        for rs, re in ivs:
            o = F32(min(he, re) - max(hs, rs)) / F32(re - rs)
            acc = max(F32(-1) + (F32(2) * o if rtok == tok else o), acc)
    return acc


def frame_phone(refs, tok, hs, he, normalization, fma):
    """FramePhoneAccuracyAutomaton::accuracy (:747-762)"""
    accs = [0] * (he - hs)
    for rtok, ivs in refs.items():
        for rs, re in ivs if rtok == tok else ():
            for i in range(max(rs - hs, 0), min(re - hs, len(accs))):
                accs[i] = 1
    return F32(F32(sum(accs)) / F32(mad32(fma, F32(normalization), F32(he - hs - 1), F32(1))))


def key_accuracy(mode, frames, key, short_pause, normalization=0.0, fma=False):
    """modifyState (:601-641; frame-state :856-879) for one key against its segment's active states"""
    _, tbeg, tokens = key
    weight = F32(0)
    if mode == "frame-state":
        for i, tok in enumerate(tokens or []):
            weight = F32(weight + F32(0 if tok in short_pause else int(tok) in frames.get(tbeg + i, {})))
        return weight
    for tok, hs, he in runs(tbeg, tokens):
        if tok in short_pause:
            continue
        refs = {}
        for t in range(hs, he):
            for rtok, ivs in frames.get(t, {}).items():
                refs.setdefault(rtok, set()).update(ivs)
        weight = F32(weight + (approximate(refs, tok, hs, he) if mode == "approximate-phone" else frame_phone(refs, tok, hs, he, normalization, fma)))
    return weight


def accuracies(mode, keys, is_reference, short_pause, normalization=0.0, fma=False):
    """-> (f32 [n_keys], {segment: active states})"""
    segs = {s: active_states([k for k, r in zip(keys, is_reference) if r and k[0] == s], mode == "frame-state") for s in {k[0] for k in keys}}
    return np.array([key_accuracy(mode, segs[k[0]], k, set(short_pause), normalization, fma) for k in keys], F32), segs
