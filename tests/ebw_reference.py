"""Plain restatement of the corpus pass of EBW training in numpy: neither the reference nor the library is called.

What is restated (reference line numbers as in include/amx.h, section "EBW"):
  sides       Lattice/Accumulator.tcc:66-87 under Speech/SegmentwiseGmmTrainer.cc:160-168: an arc is numerator if w > threshold,
              denominator with weight -w if -w > threshold; f32, strict
  collection  Accumulator.tcc:101-107 (Collector::collect): per (side, frame, mixture) the f64 sum of the widened arc weights in
              arc order, then item order.  This order is the input's, so the collected weights have ONE right value in every bit
  sums        Accumulator.tcc:109-115 -> Mm/DiscriminativeMixtureSetEstimator.cc:187-203, Mm/MixtureEstimator.cc:92-97 (numerator:
              weights_ += w), Mm/EbwDiscriminativeMixtureEstimator.cc:109-116 (denominator: denWeights_ += w; the override does not call
              Mm/DiscriminativeMixtureEstimator.cc:59-66, so weights_ is never reduced), Mm/Utilities.hh:108-153: x + w * y and
              x + w * y * y, fused under "fma"

The order of the keys is selectable, because the reference's finish() walks an unordered_map:
  "device"  ascending (frame, mixture); no cell takes keys of both sides: the library's
  "sorted"  segment by segment the denominator keys, then the numerator keys (SegmentwiseGmmTrainer.cc:164-166), each ascending
  a list    key numbers (positions in collect()'s list) in the order to take them

The flat buffer: [slot weights (weights_: numerator keys only) | mean weights | mean sums | cov weights | cov sums]
                 [denominator: slot weights | mean weights | mean sums | cov weights | cov sums] [objective]

tests/test_ebw.py holds this file to tests/golden/ref_ebw.npz (the reference's own text in both builds) in every bit, given the key order
that the fixture records.  DEFECTS are planted mistakes; tests/test_ebw.py checks that each of them leaves the fixture's check and
tests/test_ebw_gpu.py that each leaves the device's bits on the test's own problem.
"""
import math
import struct

import numpy as np

from tests.cmllr_reference import fma

EPSILON = np.float32(1.1920928955078125e-07)
DEFECTS = ("threshold-not-strict", "denominator-subtracted", "sides-swapped", "reversed-arcs")
NUM, DEN = 0, 1


def layout(model):
    nk = int(model["mix_offsets"][-1])
    n_mean, n_cov, dim = model["means"].shape[0], model["variances"].shape[0], int(model["dim"])
    o, pos = {}, 0
    for name, n in (("num_mixture_weights", nk), ("num_mean_weights", n_mean), ("num_mean_sums", n_mean * dim), ("num_cov_weights", n_cov),
                    ("num_cov_sums", n_cov * dim), ("den_density_weights", nk), ("den_mean_weights", n_mean), ("den_mean_sums", n_mean * dim),
                    ("den_cov_weights", n_cov), ("den_cov_sums", n_cov * dim), ("objective", 1)):
        o[name] = pos
        pos += n
    o["size"] = pos
    return o


def side_of(w, threshold=EPSILON, defect=None):
    """NUM, DEN or -1 for one f32 arc weight"""
    w, threshold = np.float32(w), np.float32(threshold)
    over = (lambda v: v >= threshold) if defect == "threshold-not-strict" else (lambda v: v > threshold)
    s = NUM if over(w) else (DEN if over(np.float32(-w)) else -1)
    if defect == "sides-swapped" and s >= 0:
        s = 1 - s
    return s


def collect(frame_offsets, arc_offsets, arc_weight, item_offsets, item_frame, item_emission, threshold=EPSILON, defect=None):
    """the keys in the order they are first collected: list of dict(segment, side, frame (relative to frame_offsets[0]), mixture, weight)"""
    frame_offsets = np.asarray(frame_offsets, np.int64)
    keys, index = [], {}
    for s in range(len(frame_offsets) - 1):
        arcs = range(int(arc_offsets[s]), int(arc_offsets[s + 1]))
        for a in (reversed(arcs) if defect == "reversed-arcs" else arcs):
            w = np.float32(arc_weight[a])
            side = side_of(w, threshold, defect)
            if side < 0:
                continue
            mag = float(np.float32(abs(w)))   # the denominator's fsa carries -w; the widening is exact
            for i in range(int(item_offsets[a]), int(item_offsets[a + 1])):
                f, m = int(item_frame[i]), int(item_emission[i])
                assert 0 <= f < frame_offsets[s + 1] - frame_offsets[s]
                k = (side, int(frame_offsets[s] - frame_offsets[0]) + f, m)
                if k not in index:
                    index[k] = len(keys)
                    keys.append(dict(segment=s, side=side, frame=k[1], mixture=m, weight=0.0))
                keys[index[k]]["weight"] += mag
    return keys


def key_order(keys, order):
    if isinstance(order, str):
        if order == "device":
            return sorted(range(len(keys)), key=lambda i: (keys[i]["frame"], keys[i]["mixture"], keys[i]["side"]))
        assert order == "sorted"
        return sorted(range(len(keys)), key=lambda i: (keys[i]["segment"], -keys[i]["side"], keys[i]["frame"], keys[i]["mixture"]))
    return list(order)


def accumulate(model, feats, best, keys, order="device", contract="off", acc=None, defect=None):
    """add the keys to the flat buffer.  feats [rows, dim] f32 with row 0 = frame 0 of the keys; best [rows, n_mix]: the best density
    within the mixture per (frame, mixture), 0xffffffff or anything behind the mixture's last density = none (the key is left out)"""
    o, dim = layout(model), int(model["dim"])
    acc = np.zeros(o["size"], np.float64) if acc is None else acc
    off = model["mix_offsets"].astype(np.int64)
    fused = contract == "fma"
    for i in key_order(keys, order):
        k = keys[i]
        m, j = k["mixture"], int(best[k["frame"], k["mixture"]])
        if j >= off[m + 1] - off[m]:
            continue
        slot = int(off[m] + j)
        d = int(model["dens_index"][slot])
        mean, cov = int(model["dens_mean"][d]), int(model["dens_cov"][d])
        w, y = k["weight"], feats[k["frame"]].astype(np.float64)
        p = "num" if k["side"] == NUM else "den"
        if k["side"] == NUM:
            acc[o["num_mixture_weights"] + slot] += w
        else:
            acc[o["den_density_weights"] + slot] += w
            if defect == "denominator-subtracted":   # the base class's accumulateDenominator, which the EBW class overrides without calling
                acc[o["num_mixture_weights"] + slot] -= w
        acc[o[p + "_mean_weights"] + mean] += w
        acc[o[p + "_cov_weights"] + cov] += w
        ms = acc[o[p + "_mean_sums"] + mean * dim:o[p + "_mean_sums"] + (mean + 1) * dim]
        cs = acc[o[p + "_cov_sums"] + cov * dim:o[p + "_cov_sums"] + (cov + 1) * dim]
        ms[:] = fma(w, y, ms) if fused else ms + w * y
        cs[:] = fma(w * y, y, cs) if fused else cs + (w * y) * y
    return acc


def accumulate_objective(model, acc, objective):
    acc[layout(model)["objective"]] += float(np.float32(objective))
    return acc


# ---------------------------------------------------------------------------------------------------------------- files

def _u32(v):
    return struct.pack("<I", int(v))


def _vector(sums, weight):
    """VectorAccumulator::write (Mm/VectorAccumulator.hh:91-100): the vector with its size in front, then the weight"""
    sums = np.asarray(sums, "<f8")
    return _u32(len(sums)) + sums.tobytes() + struct.pack("<d", float(weight))


def file_bytes(model, acc, version=2, plain=False):
    """EbwDiscriminativeMixtureSetEstimator::write(Core::BinaryOutputStream&): AbstractMixtureSetEstimator.cc:404-508 with the records of
    EbwDiscriminativeGaussDensityEstimator.cc:55-58 / :150-153, EbwDiscriminativeMixtureEstimator.cc:148-154 and the objective of
    DiscriminativeMixtureSetEstimator.cc:115-119.  plain: without those additions, the file of Mm::MixtureSetEstimator from the numerator block
    (what amx_gmm_accumulator_write writes, which tests/test_cache.py holds to oracle/acc_format.py)"""
    o, dim = layout(model), int(model["dim"])
    off = model["mix_offsets"].astype(np.int64)
    magic = b"MIXSET\0\0" if plain else b"DTACC\0\0\0"   # DiscriminativeMixtureSetEstimator::magic(); eight bytes are written
    out = [magic, _u32(version), _u32(dim)]
    for what, n in (("mean", model["means"].shape[0]), ("cov", model["variances"].shape[0])):
        out.append(_u32(n))
        for i in range(n):
            for p in (("num",) if plain else ("num", "den")):
                s, w = o["%s_%s_sums" % (p, what)], o["%s_%s_weights" % (p, what)]
                out.append(_vector(acc[s + i * dim:s + (i + 1) * dim], acc[w + i]))
    out.append(_u32(len(model["dens_mean"])))
    for d in range(len(model["dens_mean"])):
        out.append(_u32(model["dens_mean"][d]) + _u32(model["dens_cov"][d]))
    out.append(_u32(len(off) - 1))
    for m in range(len(off) - 1):
        out.append(_u32(off[m + 1] - off[m]))
        for k in range(off[m], off[m + 1]):
            out.append(_u32(model["dens_index"][k]) + struct.pack("<d", float(acc[o["num_mixture_weights"] + k])))
        for k in (() if plain else range(off[m], off[m + 1])):
            out.append(struct.pack("<d", float(acc[o["den_density_weights"] + k])))
    if not plain:
        out.append(struct.pack("<d", float(acc[o["objective"]])))
    return b"".join(out)


def combine(acc, add):
    """AbstractMixtureSetEstimator::accumulate(is, os) for two files: the first plus the second in every cell, the objective included"""
    return np.asarray(acc, np.float64) + np.asarray(add, np.float64)


# ---------------------------------------------------------------------------------------------------------------- estimate

F64_EPSILON, F64_DELTA, F64_MIN = 2.2204460492503131e-16, 2.2250738585072014e-308, -1.7976931348623157e+308
ESTIMATE_DEFAULTS = dict(min_observation_weight=5.0, min_relative_weight=0.0, min_variance=0.0, normalize_mixture_weights=True, type="global-rwth",
                         step_size=1.1, minimum_icd=1.0, beta=1.0, sigma_minimum=None, sigma_minimum_factor=1e-5, number_of_iterations=100,
                         i_smoothing_means=0.0, i_smoothing_weights=0.0)
ESTIMATE_DEFECTS = ("xi-branch-dropped", "sigma-minimum-missing", "ismoothing-missing-from-dtweight", "normalisation-skipped")


class Refused(Exception):
    """what amx_ebw_estimate refuses: kind "unsupported" or "invalid" """

    def __init__(self, kind, message):
        super().__init__(message)
        self.kind = kind


def _max(a, b):
    return b if a < b else a   # std::max


def log_exp_norm(v):
    """Mm/Utilities.hh:43-51: the first maximum is left out of the sum"""
    mx = 0
    for i in range(1, len(v)):
        if v[mx] < v[i]:
            mx = i
    r = 0.0
    for i in range(len(v)):
        if i != mx:
            r += math.exp(v[i] - v[mx])
    return math.log1p(r) + v[mx]


def estimate(model, acc, previous, ismoothing=None, cfg=None, contract="off", defect=None, orders=None):
    """Mm::DiscriminativeMixtureSetEstimator::estimate (Mm/DiscriminativeMixtureSetEstimator.cc:136-160) for the EBW estimators, operation by
    operation in f64: the previous (and i-smoothing) mixture set distributed by index (:51-86), the discriminative removal
    (Mm/DiscriminativeMixtureEstimator.cc:34-49, its `--densityMax` after EVERY removal included), the index maps in order of first
    appearance, Mm/IterationConstants.cc (Xi, sigma-minimum, minimumDk, global-rwth / local-rwth, set), the Cambridge mixture weights
    (Mm/EbwDiscriminativeMixtureEstimator.cc:39-91, :123-136), the means and covariances (Mm/EbwDiscriminativeGaussDensityEstimator.cc:73-99,
    :165-207, the i-smoothing variants :114-121, :222-229, Mm/ISmoothingGaussDensityEstimator.cc:56-89), the i-smoothing objective on the
    NEW set (Mm/ISmoothingMixtureSetEstimator.cc:96-115) and Mixture::removeDensitiesWithLowWeight of finalize (:92-98, Mm/Mixture.cc:109-129).

    previous / ismoothing: dict(log_weight [slots], means [n_mean, dim] f32, variances [n_cov, dim] f32) on the model's topology.
    orders (what the reference leaves to its hash tables; default ascending index): dict(cov_walk [old covariances],
    cov_densities {old covariance: [old densities]}, cov_means {old covariance: [old means]}).
    Returns dict(model, icd [new means], xi [mixtures], sigma_minimum, dk_min, dk_dim, dk_positive {new covariance: .}, clamped [(mixture,
    density in mixture)], fallback [new means], floored [(new covariance, component)], removed [(mixture, old slot)], i_objective,
    dens_old, mean_old, cov_old)."""
    c = dict(ESTIMATE_DEFAULTS)
    c.update(cfg or {})
    fused = contract == "fma"

    def mad(a, b, s):
        return fma(a, b, s) if fused else a * b + s

    o, dim = layout(model), int(model["dim"])
    acc = np.asarray(acc, np.float64)
    if not np.isfinite(acc).all():
        raise Refused("invalid", "entry %d of the accumulator is not finite" % int(np.argwhere(~np.isfinite(acc))[0][0]))
    if c["type"] == "cambridge":
        raise Refused("unsupported", "iteration constants of type cambridge: maximumRoot starts with require(false)")
    if c["type"] not in ("global-rwth", "local-rwth"):
        raise Refused("invalid", "unknown type of iteration constants")
    off = model["mix_offsets"].astype(np.int64)
    n_mix, nk = len(off) - 1, int(off[-1])
    dens_index, dens_mean, dens_cov = (model[k].astype(np.int64) for k in ("dens_index", "dens_mean", "dens_cov"))
    owner = {}
    for m in range(n_mix):
        for k in range(off[m], off[m + 1]):
            d = int(dens_index[k])
            if d in owner:
                raise Refused("unsupported", "density %d is shared by mixtures %d and %d" % (d, owner[d], m))
            owner[d] = m
    mean_owner = {}
    for d in sorted(owner):
        if int(dens_mean[d]) in mean_owner:
            raise Refused("unsupported", "mean %d is shared by densities %d and %d" % (int(dens_mean[d]), mean_owner[int(dens_mean[d])], d))
        mean_owner[int(dens_mean[d])] = d
    if c["type"] == "local-rwth":
        for m in range(n_mix):
            if len({int(dens_cov[dens_index[k]]) for k in range(off[m], off[m + 1])}) > 1:
                raise Refused("unsupported", "local-rwth: the densities of mixture %d use more than one covariance" % m)
    ism = ismoothing is not None
    cm, cw = (float(c["i_smoothing_means"]), float(c["i_smoothing_weights"])) if ism else (0.0, 0.0)
    W, DW = acc[o["num_mixture_weights"]:][:nk], acc[o["den_density_weights"]:][:nk]
    prev_w = np.array([math.exp(v) for v in np.asarray(previous["log_weight"], np.float64)])   # libm, as Mixture::weight()
    i_w = np.array([math.exp(v) for v in np.asarray(ismoothing["log_weight"], np.float64)]) if ism else None
    pm, pv = np.asarray(previous["means"], np.float32), np.asarray(previous["variances"], np.float32)
    im, iv = (np.asarray(ismoothing["means"], np.float32), np.asarray(ismoothing["variances"], np.float32)) if ism else (None, None)
    n_mean, n_cov = pm.shape[0], pv.shape[0]
    nw, dw = acc[o["num_mean_weights"]:][:n_mean], acc[o["den_mean_weights"]:][:n_mean]
    ns, ds = acc[o["num_mean_sums"]:][:n_mean * dim].reshape(n_mean, dim), acc[o["den_mean_sums"]:][:n_mean * dim].reshape(n_mean, dim)
    cs, cds = acc[o["num_cov_sums"]:][:n_cov * dim].reshape(n_cov, dim), acc[o["den_cov_sums"]:][:n_cov * dim].reshape(n_cov, dim)

    # removeDensitiesWithLowWeight: weights_ against minimum-observation-weight, the previous weight against minimum-relative-weight
    mixtures, removed = [], []
    for m in range(n_mix):
        slots = list(range(off[m], off[m + 1]))
        if slots and (c["min_observation_weight"] != 0 or c["min_relative_weight"] != 0):
            dmax = 0
            for i in range(1, len(slots)):
                if W[slots[i]] > W[slots[dmax]]:
                    dmax = i
            i = 0
            while i < len(slots):
                enough = W[slots[i]] >= c["min_observation_weight"]
                enough_rel = prev_w[slots[i]] >= c["min_relative_weight"]
                if (not enough or not enough_rel) and i != dmax:
                    removed.append((m, slots.pop(i)))
                    dmax = (dmax - 1) & 0xFFFFFFFF      # DensityIndex is u32, and the reference decrements after every removal
                else:
                    i += 1
        mixtures.append(slots)

    # MixtureSetEstimatorIndexMap: first appearance
    dens_old, mean_old, cov_old = [], [], []
    for slots in mixtures:
        for k in slots:
            d = int(dens_index[k])
            for lst, v in ((mean_old, int(dens_mean[d])), (cov_old, int(dens_cov[d])), (dens_old, d)):
                if v not in lst:
                    lst.append(v)
    new_dens, new_mean, new_cov = ({v: i for i, v in enumerate(lst)} for lst in (dens_old, mean_old, cov_old))
    slot_of = {int(dens_index[k]): (m, k) for m, slots in enumerate(mixtures) for k in slots}
    orders = orders or {}
    cov_dens = {cv: [d for d in dens_old if int(dens_cov[d]) == cv] for cv in cov_old}
    cov_means = {cv: [int(dens_mean[d]) for d in cov_dens[cv]] for cv in cov_old}
    for cv in cov_old:
        cov_dens[cv] = sorted(cov_dens[cv], key=lambda d: new_dens[d])
        cov_means[cv] = sorted(set(cov_means[cv]), key=lambda j: new_mean[j])
        if cv in orders.get("cov_densities", {}):
            assert sorted(orders["cov_densities"][cv]) == sorted(cov_dens[cv])
            cov_dens[cv] = [int(d) for d in orders["cov_densities"][cv]]
        if cv in orders.get("cov_means", {}):
            assert sorted(orders["cov_means"][cv]) == sorted(cov_means[cv])
            cov_means[cv] = [int(j) for j in orders["cov_means"][cv]]
    cov_walk = [int(v) for v in orders.get("cov_walk", cov_old)]
    assert sorted(cov_walk) == sorted(cov_old)

    def dt_weight(j):
        w = nw[j] - dw[j]
        return w + cm if ism and defect != "ismoothing-missing-from-dtweight" else w

    def dt_sum(j):
        s = ns[j] - ds[j]
        return mad(cm, im[j].astype(np.float64), s) if ism else s

    i_sum_cache = {}

    def i_sum(cv):
        if cv not in i_sum_cache:
            s = iv[cv].astype(np.float64) * float(len(cov_means[cv]))
            for j in cov_means[cv]:
                y = im[j].astype(np.float64)
                s = mad(y, y, s)
            i_sum_cache[cv] = s
        return i_sum_cache[cv]

    def cov_dt_sum(cv):
        s = cs[cv] - cds[cv]
        return mad(cm, i_sum(cv), s) if ism else s

    # Xi
    xi = []
    for slots in mixtures:
        max_abs, max_num_den = 0.0, 0.0
        for k in slots:
            j = int(dens_mean[dens_index[k]])
            a = abs(dt_weight(j))
            if max_abs < a:
                max_abs, max_num_den = a, _max(dt_weight(j) + dw[j], dw[j])
        if max_abs < max_num_den and max_num_den > 0 and defect != "xi-branch-dropped":
            den = 1 + (max_abs - 1) * max_abs / max_num_den
        else:
            den = 1.0
        xi.append(float(c["beta"]) / den)
    # sigma-minimum
    smallest = np.float32(3.40282347e+38)
    for cv in cov_walk:
        smallest = min(smallest, pv[cv].min())
    sigma = float(c["sigma_minimum"]) if c["sigma_minimum"] is not None else float(c["sigma_minimum_factor"]) * float(smallest)

    def minimum_dk(cv):
        s_min = 0.0 if defect == "sigma-minimum-missing" else sigma
        num = 0.0 - cov_dt_sum(cv)
        den = np.zeros(dim)
        pc = pv[cv].astype(np.float64)
        for d in cov_dens[cv]:
            j = int(dens_mean[d])
            m, k = slot_of[d]
            dts, dtw, p = dt_sum(j), dt_weight(j), pm[j].astype(np.float64)
            # the native build shares the product dtWeight * previousMean between t2 and t3 and hoists sigmaMinimum * dtWeight out of the
            # loop over the components, so these three are never fused; the other three sums are (read off the fixture)
            prod = dtw * p
            t2 = 2 * dts - prod
            t3 = dts - prod
            num = num + s_min * dtw
            num = mad(t2, p, num)
            num = mad(xi[m] * t3, t3, num)
            den = mad(pc - s_min, prev_w[k], den)
        with np.errstate(all="ignore"):
            ratio = num / den
        best = 0
        for i in range(1, dim):
            if ratio[best] < ratio[i]:
                best = i
        rmax = float(ratio[best])
        return (rmax if rmax > 0 else 0.0), best, rmax > 0

    step, icd = float(c["step_size"]), {}
    dk_min, dk_dim, dk_positive = {}, {}, {}
    for cv in cov_walk:
        dk_min[cv], dk_dim[cv], dk_positive[cv] = minimum_dk(cv)

    def d_k(d):
        m, k = slot_of[d]
        v = 1 / xi[m]
        v -= dt_weight(int(dens_mean[d]))
        if prev_w[k] > 0:
            v /= prev_w[k]
        return v

    if c["type"] == "global-rwth":
        b = {}
        for cv in cov_walk:
            ic = 1.0
            for d in cov_dens[cv]:
                ic = _max(ic, _max(d_k(d), dk_min[cv]))
            b[cv] = ic * step
        constant = lambda d: b[int(dens_cov[d])]   # noqa: E731
    else:
        bm = {}
        for cv in cov_walk:
            for d in cov_dens[cv]:
                m = slot_of[d][0]
                if m not in bm:
                    bm[m] = step * _max(1.0, dk_min[cv])
                bm[m] = _max(step * d_k(d), bm[m])
        constant = lambda d: bm[slot_of[d][0]]   # noqa: E731
    for cv in cov_walk:
        for d in cov_dens[cv]:
            ic = constant(d) * prev_w[slot_of[d][1]]
            ic = _max(float(c["minimum_icd"]), ic)
            if not (np.isfinite(ic) and ic >= 0):
                raise Refused("invalid", "the iteration constant of density %d is %r" % (d, ic))
            icd[int(dens_mean[d])] = float(ic)

    # mixture weights
    normalize, n_iter = bool(c["normalize_mixture_weights"]), int(c["number_of_iterations"])
    log_weights, clamped = [], []
    for m, slots in enumerate(mixtures):
        n = len(slots)
        total = 0.0
        for k in slots:
            total += W[k]

        def weight(k):
            return mad(i_w[k], cw, W[k]) if ism else W[k]

        if n > 1 and total > F64_EPSILON:
            w, k_max = [], 0.0
            for k in slots:
                w.append(float(prev_w[k]))
                if w[-1] > F64_EPSILON:
                    k_max = _max(k_max, DW[k] / w[-1])
                else:
                    w[-1] = 0.0
            kk = [k_max - DW[k] / w[i] if w[i] > 0 else 0.0 for i, k in enumerate(slots)]
            for it in range(n_iter):
                for i, k in enumerate(slots):
                    if w[i] > 0:
                        w[i] = float(mad(kk[i], w[i], weight(k)))
                    if w[i] < 0:
                        w[i] = 0.0
                        if (m, i) not in clamped:
                            clamped.append((m, i))
                if normalize and defect != "normalisation-skipped":
                    s = 0.0
                    for v in w:
                        s += v
                    w = [v / s for v in w] if s > F64_DELTA else [1 / float(n)] * n
        else:
            w = [1 / float(n) if normalize else 1.0] * n
        lw = [math.log(v) if v > 0 else F64_MIN for v in w]
        if normalize and lw:
            norm = log_exp_norm(lw)
            lw = [v - norm for v in lw]
        log_weights.append(lw)

    # means
    means, fallback = np.zeros((len(mean_old), dim), np.float32), []
    for n, j in enumerate(mean_old):
        weight_j = dt_weight(j) + icd[j]
        if weight_j > 0:
            means[n] = (mad(icd[j], pm[j].astype(np.float64), dt_sum(j)) / weight_j).astype(np.float32)
        else:
            means[n] = pm[j]
            fallback.append(n)
    # covariances
    variances, floored = np.zeros((len(cov_old), dim), np.float32), []
    min_var = np.float32(c["min_variance"])
    for n, cv in enumerate(cov_old):
        buf, weight_c = np.array(cov_dt_sum(cv), np.float64), 0.0
        for j in cov_means[cv]:
            tmp = dt_weight(j) + icd[j]
            weight_c += tmp
            mean = means[new_mean[j]].astype(np.float64)
            prev_sum = pv[cv].astype(np.float64)
            prev_sum = prev_sum + (pm[j] * pm[j]).astype(np.float64)          # MeanType * MeanType: an f32 product
            prev_sum = prev_sum * icd[j]
            if fused:
                buf = buf + fma(-(tmp * mean), mean, prev_sum)
            else:
                buf = buf + (prev_sum - tmp * mean * mean)
        if not weight_c > 0:
            raise Refused("invalid", "covariance %d: the summed weight %r is not positive" % (cv, weight_c))
        v32 = (buf / weight_c).astype(np.float32)
        if not (v32 > 0).all():
            raise Refused("invalid", "covariance %d: component %d of the estimated variance is not positive" % (cv, int(np.argwhere(~(v32 > 0))[0][0])))
        if min_var != 0:
            for i in np.nonzero(v32 < min_var)[0]:
                floored.append((n, int(i)))
            v32 = np.where(v32 < min_var, min_var, v32)
        variances[n] = v32

    # the i-smoothing objective: the new set is distributed as the previous one
    i_objective = None
    if ism:
        of_w = 0.0
        for m, slots in enumerate(mixtures):
            s = 0.0
            for i, k in enumerate(slots):
                pw = math.exp(log_weights[m][i])
                s = float(mad(i_w[k], math.log(_max(pw, F64_DELTA)), s))
            of_w += cw * s
        of_m = 0.0
        for n, cv in enumerate(cov_old):
            s, size = 0.0, float(len(cov_means[cv]))
            isum = i_sum(cv)
            for i in range(dim):
                sig = variances[n, i]
                s = float(mad(size, math.log(2 * math.pi * float(sig)), s))
                t = float(isum[i])
                for j in cov_means[cv]:
                    p = means[new_mean[j], i]
                    t += float(p * (p - np.float32(2) * im[j, i]))               # f32 arithmetic throughout
                s += t / float(sig)
            of_m += -0.5 * cm * s
        i_objective = of_w + of_m

    # finalize: Mixture::removeDensitiesWithLowWeight on the new set.  densityIndexWithMaxWeight() there compares two iterators and
    # returns the number of densities, so no density is protected
    out_slots = [list(s) for s in mixtures]
    if c["min_relative_weight"] != 0:
        for m in range(n_mix):
            lw = log_weights[m]
            if not lw:
                continue
            limit = math.exp(log_exp_norm(lw)) * c["min_relative_weight"]
            i = 0
            while i < len(lw):
                if math.exp(lw[i]) < limit:
                    lw.pop(i)
                    out_slots[m].pop(i)
                else:
                    i += 1
            if normalize and lw:
                norm = log_exp_norm(lw)
                log_weights[m] = [v - norm for v in lw]
    out = dict(dim=dim, mix_offsets=np.concatenate([[0], np.cumsum([len(s) for s in out_slots])]).astype(np.uint32),
               dens_index=np.array([new_dens[int(dens_index[k])] for s in out_slots for k in s], np.uint32),
               log_weight=np.array([v for lw in log_weights for v in lw], np.float64),
               dens_mean=np.array([new_mean[int(dens_mean[d])] for d in dens_old], np.uint32),
               dens_cov=np.array([new_cov[int(dens_cov[d])] for d in dens_old], np.uint32), means=means, variances=variances)
    return dict(model=out, icd=np.array([icd[j] for j in mean_old]), xi=np.array(xi), sigma_minimum=sigma,
                dk_min=np.array([dk_min[cv] for cv in cov_old]), dk_dim=np.array([dk_dim[cv] for cv in cov_old]),
                dk_positive=np.array([dk_positive[cv] for cv in cov_old]), clamped=clamped, fallback=fallback, floored=floored, removed=removed,
                i_objective=i_objective, dens_old=np.array(dens_old), mean_old=np.array(mean_old), cov_old=np.array(cov_old))
