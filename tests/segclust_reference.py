"""Plain numpy restatement of Signal/SegmentClustering.{hh,cc} for the model CorrFullCovMonoGaussianModel: f64 throughout, np.linalg for the
inverse and the log-determinant, f32 casts exactly where the reference narrows (the 1.0F / n division, the likelihood, R, the logSum rule,
the features, the distances, the scores).  cluster() takes an optional forced merge list, so that a device run can be replayed through it."""
import numpy as np

f32, f64 = np.float32, np.float64
LN_2PI = 1.83787706640934533908193770912475883960723876953125
MINLOGEPS = f32(11.513)


class Model:
    def __init__(self, n, mean, var):
        self.n, self.mean, self.var = int(n), mean, var
        self.logdet = np.linalg.slogdet(var)[1]
        self.like = f32(f32(self.logdet) * f32(self.n))   # likelihood_ is an f32: narrowed, then *= nFrames_


def sums(x):
    """frame-order f64 chains of one segment [n, D] f32 -> (sum [D], square sum [D, D])"""
    s, q = np.zeros(x.shape[1]), np.zeros((x.shape[1], x.shape[1]))
    for row in x.astype(f64):
        s += row
        q += np.outer(row, row)
    return s, q


def singular(var):
    try:
        np.linalg.inv(var)
        return False
    except np.linalg.LinAlgError:
        return True


def finalize(x):
    """-> (Model, rounds of the +0.1 loop)"""
    s, q = sums(x)
    inv = f64(f32(1.0) / f32(len(x)))
    mean = s * inv
    var = q * inv - np.outer(mean, mean)
    bumps = 0
    while singular(var):
        var = var + 0.1 * np.eye(len(mean))
        bumps += 1
    return Model(len(x), mean, var), bumps


def relative_likelihoods(models, originals):
    """R[i][j] = relativeLikelihood of models[i] given originals[j], f32"""
    D = len(originals[0].mean)
    inv = [np.linalg.inv(m.var) for m in originals]
    R = np.zeros((len(models), len(originals)), f32)
    for i, a in enumerate(models):
        for j, b in enumerate(originals):
            d = a.mean - b.mean
            v = 0.0 - b.logdet - np.sum(inv[j] * a.var.T) - d @ inv[j] @ d - D * LN_2PI
            R[i, j] = f32(v * 0.5 * a.n)
    return R


def log_sum(v):
    """Math::Vector<f32>::logSum"""
    s = v[0]
    for x in v[1:]:
        diff = f32(s - x)
        if diff > MINLOGEPS:
            pass
        elif diff < -MINLOGEPS:
            s = x
        elif diff < 0:
            s = f32(f64(x) + np.log(1.0 + np.exp(f64(diff))))
        else:
            s = f32(f64(s) + np.log(1.0 + np.exp(-f64(diff))))
    return s


def average(R, alpha):
    total = f32(0)
    for i in range(len(R)):
        v = R[i] * f32(alpha)
        total = f32(f64(total) + np.exp(f64(f32(v[i] - log_sum(v)))))
    return f32(total / f32(len(R)))


def auto_alpha(R, minalpha=0.40, maxalpha=0.60):
    """-> (alpha, the averages the bisection saw)"""
    lo, hi, alpha, step, avg, seen = f32(minalpha), f32(maxalpha), f32(0), f32(0.5), f32(0), []
    while (avg < lo or avg > hi) and step.view(np.uint32) > 100:
        alpha = f32(alpha + step) if avg < lo else f32(alpha - step)
        step = f32(step / 2.0)
        avg = average(R, alpha)
        seen.append(avg)
    return alpha, seen


def feature(r, alpha):
    v = r * f32(alpha)
    return np.exp((v - log_sum(v)).astype(f64)).astype(f32)


def distance(fx, fy):
    return f32(-np.add.accumulate(fx * fy, dtype=f32)[-1])


def merge(x, y):
    n = x.n + y.n
    mean = (x.mean * x.n + y.mean * y.n) * f64(f32(1.0) / f32(n))
    var = (np.outer(x.mean - mean, x.mean - mean) + x.var) * (x.n / n)
    var = var + (np.outer(y.mean - mean, y.mean - mean) + y.var) * (y.n / n)
    m = Model(n, mean, var)
    return m, f32(f32(0.5) * f32(f32(m.like - x.like) - y.like))


def threshold(param, D, lam, total_frames):
    p = f32(f32(0.25) * f32(D)) * f32(f32(3) + f32(D))
    return f32(f32(param) + f32(f32(p * f32(lam)) * np.log(f32(total_frames))))


def initial_distances(F):
    N = len(F)
    dist = np.zeros((N, N), f32)
    for i in range(N):
        for j in range(i):
            dist[i, j] = distance(F[i], F[j])
    return dist


def cluster(models, R, alpha, thr, amalgamation=0, forced=None):
    """The merge loop.  -> (tracker [(parent, child, score)], picks [(distance of the merged pair, the loop's own minimum)], the largest
    |likelihood| of a model).  forced: the (parent, child) pairs to merge instead of the loop's own choice."""
    N = len(models)
    slot = list(models)
    F = [feature(R[i], alpha) for i in range(N)]
    dist = initial_distances(F)
    active = np.ones(N, bool)
    tracker, picks, lmax = [], [], max(abs(m.like) for m in models)
    for step in range(N - 1):
        cand = np.where(np.tril(np.outer(active, active), -1), dist, np.inf)
        c, p = np.unravel_index(np.argmin(cand), cand.shape)   # the first minimum in row-major order
        own = cand[c, p]
        if forced is not None:
            p, c = forced[step]
        picks.append((dist[c, p], own))
        slot[p], glr = merge(slot[p], slot[c])
        active[c], lmax = False, max(lmax, abs(slot[p].like))
        tracker.append((int(p), int(c), f32(glr - thr)))
        if amalgamation == 1:
            for i in np.flatnonzero(active):
                if i != p:
                    a, b = (max(i, p), min(i, p)), (max(i, c), min(i, c))
                    dist[a] = max(dist[a], dist[b])
        else:
            F[p] = feature(relative_likelihoods([slot[p]], models)[0], alpha)
            for i in np.flatnonzero(active):
                if i != p:
                    dist[max(i, p), min(i, p)] = distance(F[i], F[p])
    return tracker, picks, lmax


def choose(tracker, N, mincluster=2, maxcluster=100000):
    """findBestBIC and returnClustering -> (class ids as slot indices, best index, the cumulative scores the search saw)"""
    best, best_score, current, seen = -1, f32(0), f32(0), []
    if N > maxcluster:
        best = N - maxcluster - 1
    for i in range(best + 1, N - mincluster):
        current = f32(current + tracker[i][2])
        seen.append(current)
        if current < best_score:
            best_score, best = current, i
    live, ids = np.ones(N, bool), np.arange(N)
    for p, c, _ in tracker[:best + 1]:
        live[c], ids[c] = False, p
    for i in range(N - 1, 0, -1):
        j = i
        while not live[j]:
            j = ids[j]
        ids[i] = j
    return ids, best, seen
