#!/usr/bin/env python3
"""tests/golden/make_linseg_golden.py -- writes tests/golden/ref_linseg.npz: linear-segmentation alignments as Speech::LinearSegmenter
computes them (what Speech::AlignmentWithLinearSegmentationNode runs), from the reference's own text.

Run it where the reference tree is mounted; tests read only the fixture.  What it compiles, in both of the reference's arithmetics (the
flag sets of oracle/ref/Makefile: -msse3 = contract=off, -msse3 -march=native = contract=fma), taken by line range + SHA-256 into a
temporary directory that is deleted afterwards:
  * Speech/AlignmentWithLinearSegmentation.cc:30-79 (class LinearSegmenter::Delimiter with reset, feed, nFeatures), 103-120 (logLikelihood),
    145-182 (Delimiter::getDelimitation), 186-245 (SietillDelimiter), 283-285 (LinearSegmenter::nFeatures) and 315-350 (getAlignment)
behind a shell of this file's own that holds no reference text: stand-ins for Core::Component (error, warning, respondToDelayedErrors,
select), Core::Configuration and the parameter classes, the XML channel (open, and it keeps the numbers the delimiter reports: that is how
x_min leaves getDelimitation), Alignment / AlignmentItem, Fsa::InvalidLabelId, the frame of class LinearSegmenter and the two constructors,
which take the parameter values from the driver.

The cases are tests/linseg_reference.py's cases().  Recorded per case and build: the bits of M_ and Q_, the delimitation, x_min (DBL_MAX
where getDelimitation reports none), the item list or its rejection and why, and for the cases of at most 24 frames the whole
logLikelihood(ib, ie) table.  Findings (printed by every run, kept in the fixture):
  * fma_differs: which recorded arrays the -march=native build computes differently, and which of the candidate sites hold a fused
    multiply-add there.  feed's xx * xx + f / 2 cannot tell: xx is a widened f32, its square is exact in f64, and the fused and the
    plain form round the same sum once.  xsil + xspe can: the restatement is run plain and with either product fused, and exactly one
    form must reproduce the native build in every bit.
  * every case not named tie_* is DECIDED under both builds (asserted): no comparison of its search comes closer than 2^-48 S.
  * mismatch: a state count that gives "index mismatch" exists (N = 1 with two states: one frame takes index 0, the last state is 1).

    python3 tests/golden/make_linseg_golden.py [out.npz]
"""
import ctypes as C
import hashlib
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import linseg_reference as lr  # noqa: E402

REF = "/root/reference/src"
FN = "Speech/AlignmentWithLinearSegmentation.cc"
PIECES = {
    "delimiter_class": [(FN, 30, 79)],
    "log_likelihood": [(FN, 103, 120)],
    "get_delimitation": [(FN, 145, 182)],
    "sietill": [(FN, 186, 245)],
    "n_features": [(FN, 283, 285)],
    "get_alignment": [(FN, 315, 350)],
}
SHA = "05820b099dcddb90859a36530e2a959552bc45804035e66ad360c4d105c07ee3"
TABLE_MAX_FRAMES = 24

SOURCE = r'''
#include <Core/Assertions.hh>
#include <Core/Types.hh>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
// ---- shell: stand-ins (no reference text) ----
static int    g_errors, g_warnings, g_reported;
static double g_frames, g_begin, g_end, g_score;
namespace Core {
struct Configuration {
    int    iterations;
    double penalty;
    float  proportion;
    int    minimum, maximum;
};
struct ParameterInt {};
struct ParameterFloat {};
struct ParameterBool {};
struct XmlOpen {
    XmlOpen(const char*) {}
};
struct XmlClose {
    XmlClose(const char*) {}
};
struct XmlFull {
    const char* name;
    double      value;
    template<class T> XmlFull(const char* n, const T& v) : name(n), value((double)v) {}
};
class XmlChannel {
public:
    XmlChannel(const Configuration&, const char*) {}
    bool        isOpen() const { return true; }
    XmlChannel& operator<<(const XmlOpen&) { return *this; }
    XmlChannel& operator<<(const XmlClose&) {
        ++g_reported;
        return *this;
    }
    XmlChannel& operator<<(const XmlFull& f) {
        if (!std::strcmp(f.name, "frames"))
            g_frames = f.value;
        else if (!std::strcmp(f.name, "speech-begin"))
            g_begin = f.value;
        else if (!std::strcmp(f.name, "speech-end"))
            g_end = f.value;
        else if (!std::strcmp(f.name, "score"))
            g_score = f.value;
        return *this;
    }
};
class Component {
public:
    Configuration config;
    Component(const Configuration& c) : config(c) {}
    virtual ~Component() {}
    void          error(const char*, ...) const { ++g_errors; }
    void          warning(const char*, ...) const { ++g_warnings; }
    void          respondToDelayedErrors() const {}
    Configuration select(const char*) const { return config; }
};
}  // namespace Core
namespace Fsa {
typedef s32 LabelId;
static const LabelId InvalidLabelId = 2147483647;
}  // namespace Fsa
namespace Am {
typedef s32 AllophoneStateIndex;
}
namespace Speech {
typedef u32 TimeframeIndex;
struct AlignmentItem {
    TimeframeIndex          time;
    Am::AllophoneStateIndex emission;
    AlignmentItem(TimeframeIndex t, Am::AllophoneStateIndex e) : time(t), emission(e) {}
};
typedef std::vector<AlignmentItem> Alignment;
// the frame of class LinearSegmenter: the members its pieces below use
class LinearSegmenter : public Core::Component {
public:
    class Delimiter;
    Delimiter*                           delimiter_;
    Am::AllophoneStateIndex              silence_;
    std::vector<Am::AllophoneStateIndex> states_;
    u32                                  minimumSegmentLength_, maximumSegmentLength_;
    const u32                            maximumJump_;
    LinearSegmenter(const Core::Configuration&, bool sietill);
    bool getAlignment(Alignment&) const;
    u32  nFeatures() const;
};
}  // namespace Speech
using namespace Speech;
// ---- reference text: class LinearSegmenter::Delimiter ----
%(delimiter_class)s
// ---- shell: the constructor with the parameters' values handed in by the driver
LinearSegmenter::Delimiter::Delimiter(const Core::Configuration& c)
        : Core::Component(c), numberOfIterations_(c.iterations), f_(c.penalty), minimumSpeechProportion_(c.proportion), statisticsChannel_(c, "statistics") {}
// ---- reference text: logLikelihood ----
%(log_likelihood)s
// ---- reference text: Delimiter::getDelimitation ----
%(get_delimitation)s
// ---- reference text: SietillDelimiter ----
%(sietill)s
// ---- shell
LinearSegmenter::LinearSegmenter(const Core::Configuration& c, bool sietill)
        : Core::Component(c), delimiter_(0), silence_(Fsa::InvalidLabelId), minimumSegmentLength_(c.minimum), maximumSegmentLength_(c.maximum), maximumJump_(2) {
    if (sietill)
        delimiter_ = new SietillDelimiter(select("delimiter"));
    else
        delimiter_ = new Delimiter(select("delimiter"));
}
// ---- reference text: LinearSegmenter::nFeatures ----
%(n_features)s
// ---- reference text: LinearSegmenter::getAlignment ----
%(get_alignment)s
// ---- this generator's own driver (no reference text) ----
// One segment.  Outputs: M, Q [N + 1]; out[0..8] = valid, accepted, begin, end, reported (getDelimitation wrote its statistics), errors,
// warnings, items, times in order; score; label [N] (-1 where no item); table [(N + 1) x (N + 1)] or NULL.
extern "C" void ref_linseg(int N, const float* energy, int n_states, const int* labels, int silence, int sietill, int iterations, double penalty,
                           float proportion, int minimum, int maximum, double* M, double* Q, int* out, double* score, int* label, double* table) {
    Core::Configuration c;
    c.iterations = iterations, c.penalty = penalty, c.proportion = proportion, c.minimum = minimum, c.maximum = maximum;
    g_errors = g_warnings = g_reported = 0;
    LinearSegmenter seg(c, sietill != 0);
    seg.silence_ = silence;
    seg.delimiter_->reset();                 // setModel (:294-295)
    seg.states_.assign(labels, labels + n_states);
    for (int t = 0; t < N; ++t) {
        const f32 f = energy[t];
        seg.delimiter_->feed(f);             // LinearSegmenter::feed(f32) (:307-309): widened by the call
    }
    for (int i = 0; i <= N; ++i)
        M[i] = seg.delimiter_->M_[i], Q[i] = seg.delimiter_->Q_[i];
    for (int t = 0; t < N; ++t)
        label[t] = -1;
    for (int i = 0; i < 9; ++i)
        out[i] = 0;
    out[2] = out[3] = -1;
    out[5] = g_errors;
    *score = DBL_MAX;
    const bool valid = seg.states_.size() > 0 && seg.nFeatures() > 0;   // isAlignmentValid (:311-313)
    out[0] = valid;
    if (!valid || g_errors)
        return;
    if (table)
        for (u32 ib = 1; ib <= (u32)N; ++ib)
            for (u32 ie = ib; ie <= (u32)N; ++ie)
                table[(size_t)ib * (N + 1) + ie] = seg.delimiter_->logLikelihood(ib, ie);
    if (seg.nFeatures() >= seg.minimumSegmentLength_ && seg.nFeatures() <= seg.maximumSegmentLength_) {
        std::pair<TimeframeIndex, TimeframeIndex> d = seg.delimiter_->getDelimitation();
        out[2] = (int)d.first, out[3] = (int)d.second;
        out[4] = g_reported;
        if (g_reported)
            *score = g_score;
        g_warnings = 0;
    }
    Alignment a;
    out[1] = seg.getAlignment(a);
    out[6] = g_warnings;
    out[7] = (int)a.size();
    out[8] = 1;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].time != i || i >= (size_t)N)
            out[8] = 0;
        else
            label[i] = a[i].emission;
    }
}
'''

FLAGS = ["-std=c++20", "-O2", "-msse3", "-fPIC", "-funsigned-char", "-fno-strict-aliasing", "-fno-access-control", "-D_GNU_SOURCE", "-DSPRINT_RELEASE_BUILD",
         "-I" + REF, "-I/usr/include/libxml2", "-w"]
FIELDS = ("M", "Q", "begin", "end", "score", "reason", "label", "emission", "n_items")


def reference_text():
    cache, parts, h = {}, {}, hashlib.sha256()
    for key, ranges in PIECES.items():
        out = []
        for fn, first, last in ranges:
            if fn not in cache:
                with open(os.path.join(REF, fn), encoding="utf-8", errors="replace") as f:
                    cache[fn] = f.readlines()
            out.append("".join(cache[fn][first - 1:last]))
        parts[key] = "\n".join(out)
        h.update(parts[key].encode())
    return parts, h.hexdigest()


def build(tmp, flavour, parts):
    gen = os.path.join(tmp, "linseg_%s.cc" % flavour)
    with open(gen, "w") as f:
        f.write(SOURCE % parts)
    so = os.path.join(tmp, "linseg_%s.so" % flavour)
    extra = [] if flavour == "off" else ["-march=native"]
    subprocess.check_call(["g++"] + FLAGS + extra + ["-shared", "-o", so, gen])
    fma = subprocess.run("objdump -d %s | grep -c -E 'vfn?m(add|sub)'" % so, shell=True, capture_output=True, text=True).stdout.strip()
    L = C.CDLL(so)
    L.ref_linseg.restype = None
    return L, int(fma or 0)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(L, cases):
    a = {}
    for name, c in cases.items():
        cfg = dict(lr.DEFAULTS)
        cfg.update(c["cfg"])
        e, lab, emi = np.ascontiguousarray(c["energy"], np.float32), np.ascontiguousarray(c["labels"], np.int32), c["emissions"]
        N = len(e)
        M, Q, out, score, label = np.zeros(N + 1), np.zeros(N + 1), np.zeros(9, np.int32), np.zeros(1), np.zeros(N, np.int32)
        table = np.zeros((N + 1, N + 1)) if N <= TABLE_MAX_FRAMES else None
        L.ref_linseg(N, p(e), len(lab), p(lab), lr.SILENCE_LABEL, int(cfg["should_use_sietill"]), int(cfg["number_of_iterations"]), C.c_double(cfg["penalty"]),
                     C.c_float(cfg["minimum_speech_proportion"]), int(cfg["minimum_segment_length"]), int(cfg["maximum_segment_length"]), p(M), p(Q),
                     p(out), p(score), p(label), p(table) if table is not None else None)
        valid, accepted, begin, end, reported, errors, warnings, items, in_order = (int(v) for v in out)
        assert not errors, "%s: the reference raised an error" % name
        if not valid:
            reason = lr.NO_STATES
        elif N < cfg["minimum_segment_length"]:
            reason = lr.TOO_SHORT
        elif N > cfg["maximum_segment_length"]:
            reason = lr.TOO_LONG
        elif accepted:
            reason = lr.OK
        else:
            reason = lr.MISMATCH if warnings else lr.JUMP   # only the mismatch is warned about (:341)
        assert (items == N and in_order) if accepted else items == 0, "%s: %d items for %d frames" % (name, items, N)
        assert accepted == (reason == lr.OK) and (reason in (lr.NO_STATES, lr.TOO_SHORT, lr.TOO_LONG)) == (begin < 0), name
        to_emission = {int(l): int(x) for l, x in zip(lab, emi)}
        to_emission[lr.SILENCE_LABEL] = lr.SILENCE_EMISSION
        k = name + "/"
        a[k + "M"], a[k + "Q"] = M, Q
        a[k + "begin"], a[k + "end"], a[k + "score"] = np.array(begin, np.int32), np.array(end, np.int32), score[0].copy()
        a[k + "reason"], a[k + "n_items"] = np.array(reason, np.int32), np.array(items, np.int32)
        a[k + "label"] = label
        a[k + "emission"] = np.array([to_emission[int(l)] if l >= 0 else -1 for l in label], np.int32)
        if table is not None and valid:
            a[k + "table"] = table
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def restated(cases, contract, sites=None, names=None):
    a = {}
    for name, c in cases.items():
        if names is not None and name not in names:
            continue
        N = len(c["energy"])
        r = lr.segment(c["energy"], c["labels"], c["emissions"], contract=contract, sites=sites, table=N <= TABLE_MAX_FRAMES, **c["cfg"])
        k = name + "/"
        if r["M"] is not None:
            a[k + "M"], a[k + "Q"] = r["M"], r["Q"]
        a[k + "begin"], a[k + "end"], a[k + "score"] = np.array(r["begin"], np.int32), np.array(r["end"], np.int32), np.float64(r["score"])
        a[k + "reason"], a[k + "label"], a[k + "emission"] = np.array(r["reason"], np.int32), r["label"], r["emission"]
        if r["table"] is not None:
            a[k + "table"] = r["table"]
        a[k + "decided"] = np.array(r["decided"])
    return a


def differences(want, got):
    """keys of `got` (but 'decided') whose bits are not `want`'s"""
    return [k for k, v in got.items() if not k.endswith("/decided") and not same_bits(np.asarray(v), np.asarray(want[k]))]


def write_npz(path, arrays):
    """numpy.savez_compressed with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "ref_linseg.npz")
    parts, sha = reference_text()
    if "--print-sha" in sys.argv:
        print(sha)
        return
    if sha != SHA:
        sys.exit("make_linseg_golden: the reference text hashes to %s, expected %s -- re-check the line ranges" % (sha, SHA))
    cases = lr.cases()
    arrays = {}
    for name, c in cases.items():
        cfg = dict(lr.DEFAULTS)
        cfg.update(c["cfg"])
        arrays["in/%s/energy" % name] = np.ascontiguousarray(c["energy"], np.float32)
        arrays["in/%s/labels" % name], arrays["in/%s/emissions" % name] = c["labels"].astype(np.int32), c["emissions"].astype(np.int32)
        arrays["cfg/" + name] = np.array([cfg[k] for k in ("number_of_iterations", "penalty", "minimum_speech_proportion", "should_use_sietill",
                                                           "minimum_segment_length", "maximum_segment_length")], np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for fl in ("off", "fma"):
            L, n_fma = build(tmp, fl, parts)
            arrays["fma_instructions/" + fl] = np.array(n_fma)
            got[fl] = run(L, cases)
    for k, v in got["off"].items():
        arrays["off/" + k] = v
    differ = [k for k, v in got["fma"].items() if not same_bits(v, got["off"][k])]
    for k in differ:
        arrays["fma/" + k] = got["fma"][k]
    arrays["fma_differs"] = np.array(differ if differ else [""])
    arrays["fma_arrays_compared"] = np.array(len(got["fma"]))
    # the restatement without fused sites is the -msse3 build
    off = restated(cases, "off")
    bad = differences(got["off"], off)
    assert not bad, "the restatement (contract=off) differs from the reference in %s" % bad[:8]
    # which sites the native build fuses: exactly one combination reproduces it
    small = [n for n, c in cases.items() if len(c["energy"]) <= 129]
    fits = [s for s in (None, "xsil", "xspe") if not differences(got["fma"], restated(cases, "fma", dict(sum=s), small))]
    assert fits == [lr.FMA_SITES["sum"]], "fused forms of xsil + xspe that reproduce the -march=native build: %s" % fits
    arrays["fma_sites"] = np.array(["sum=%s" % fits[0]])
    fma = restated(cases, "fma")
    bad = differences(got["fma"], fma)
    assert not bad, "the restatement (contract=fma) differs from the reference in %s" % bad[:8]
    undecided = sorted(n for n in cases for r in (off, fma) if not r[n + "/decided"])
    assert all(lr.is_tie(n) for n in undecided), "cases that are not decided: %s" % undecided
    arrays["undecided"] = np.array(sorted(set(undecided)) or [""])
    for n in cases:
        arrays["decided/" + n] = np.array([bool(off[n + "/decided"]), bool(fma[n + "/decided"])])
    reasons = {n: int(got["off"][n + "/reason"]) for n in cases}
    assert reasons["d_mismatch_n1"] == lr.MISMATCH and reasons["d_states_jump"] == lr.JUMP and reasons["d_minimum_below"] == lr.TOO_SHORT
    assert reasons["d_maximum_above"] == lr.TOO_LONG and reasons["d_minimum_at"] == lr.OK and reasons["d_maximum_at"] == lr.OK
    assert got["off"]["d_gate_none/score"] == lr.DBL_MAX and got["off"]["d_quiet_speech/score"] == lr.DBL_MAX
    write_npz(out, arrays)
    print("%s: %d arrays, %d bytes" % (out, len(arrays), os.path.getsize(out)))
    print("  fma instructions: off %d, fma %d" % (int(arrays["fma_instructions/off"]), int(arrays["fma_instructions/fma"])))
    print("  fma copies that differ from off: %d of %d" % (len(differ), len(got["fma"])))
    print("    by field: %s" % {f: sum(1 for k in differ if k.endswith("/" + f)) for f in FIELDS + ("table",)})
    print("  fused site of the native build: xsil + xspe with the product %s fused into the sum" % fits[0])
    print("  not decided: %s" % sorted(set(undecided)))
    print("  reasons: %s" % {lr.REASONS[r]: sum(1 for v in reasons.values() if v == r) for r in sorted(set(reasons.values()))})


if __name__ == "__main__":
    main()
