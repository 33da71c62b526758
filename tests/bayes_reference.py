"""Plain restatement of the reference's Bayes classification (Signal/BayesClassification.cc, LikelihoodFunction.cc, AprioriProbability.cc):
numpy, f32 throughout, the frame loop in Python, vectorised over classes only.  tests/test_bayes.py holds it against the reference's own
results (tests/golden/ref_bayes.npz) bit for bit; the GPU tests hold the library against it.

It replays the two nodes' work loops frame by frame and keeps the reference's state (nFeatures_, nFeaturesBuffered_, newData_, the
window as a list with the newest element first) instead of closed forms, so that the device code's closed forms are checked against
something that does not share them.
"""
import numpy as np

INT_MAX = 2 ** 31 - 1
F32_MAX = np.finfo(np.float32).max


def prior(n_classes):
    """UniformAprioriProbability::setClasses (AprioriProbability.cc:20): std::log of an f32, the float overload"""
    return np.log(np.float32(n_classes))


def arg_min(scores):
    """BayesClassification::argMin (:138-157): strict < from Type<f32>::max, so the first minimum wins and a NaN or a value >= max never
    does; -1 where the reference would index out of range"""
    best, label = F32_MAX, -1
    for c, s in enumerate(scores):
        if s < best:
            best, label = s, c
    return label


class Classifier:
    """one BayesClassification object: feed / classify / getScores / reset with the reference's members"""

    def __init__(self, n_classes, number_of_features=INT_MAX, delay=INT_MAX, window_length=-1, window_right=0, oldest_first=False):
        self.n = int(n_classes)
        self.n_used = INT_MAX if number_of_features <= 0 or number_of_features >= INT_MAX else int(number_of_features)
        self.delay = INT_MAX if delay < 0 or delay >= INT_MAX else int(delay)
        self.window = int(window_length) if window_length > 0 else 0
        if self.window and window_right >= self.window:
            raise ValueError("window_right %d must be smaller than window_length %d" % (window_right, self.window))
        self.oldest_first = oldest_first      # NOT the reference: the order test's other order
        self.log_n = prior(self.n)
        self.reset()

    def reset(self):
        self.sums = np.zeros(self.n, np.float32)
        self.sum_of_weights = np.float32(0)
        self.win = []
        self.n_features = self.n_buffered = 0
        self.new_data = False

    def feed(self, row, w):
        s = (np.float32(w) * np.asarray(row, np.float32)).astype(np.float32)   # LikelihoodFunction.cc:77, rounded once
        self.sums = (self.sums + s).astype(np.float32)                          # :80
        self.sum_of_weights = np.float32(self.sum_of_weights + np.float32(w))   # LikelihoodFunction.hh:55
        if self.window:
            self.win.insert(0, s)                                               # SlidingWindow::add: push_front, drop the oldest
            del self.win[self.window:]
        self.n_features += 1
        self.n_buffered += 1
        self.new_data = True

    def class_scores(self):
        """argMin's per-class scores (:143-150)"""
        score = np.full(self.n, self.log_n, np.float32)
        if self.window:
            for s in (reversed(self.win) if self.oldest_first else self.win):
                score = (score + s).astype(np.float32)
        else:
            score = (score + self.sums).astype(np.float32)
        return score

    def classify(self):
        """:80-101 -> (label, per-class scores) or None"""
        if not self.new_data:
            return None
        sc = self.class_scores()
        self.n_buffered = 0
        self.new_data = False
        return arg_min(sc), sc

    def classify_frame(self, row, w):
        """:103-119"""
        self.feed(row, w)
        output = self.n_features >= self.n_used
        if not self.window and self.n_features > self.delay:
            output = True
        if self.window and len(self.win) == self.window and (self.delay == INT_MAX or self.n_buffered >= self.delay):
            output = True
        return self.classify() if output else None

    def get_scores(self):
        """:121-133: the cumulative sums, never the window"""
        if not self.new_data:
            return None
        self.new_data = False
        return (np.full(self.n, self.log_n, np.float32) + self.sums).astype(np.float32)

    def get_scores_frame(self, row, w):
        """:182-189"""
        self.feed(row, w)
        return self.get_scores() if self.n_features > self.delay else None


def check_weights(weights):
    """BayesClassificationNode::featureScoreWeight (:369-372): the first frame whose weight is not >= 0, or -1"""
    bad = np.nonzero(~(np.asarray(weights, np.float32) >= 0))[0]
    return int(bad[0]) if len(bad) else -1


def classify_segment(scores, weights=None, **cfg):
    """BayesClassificationNode::work (:384-411) over one segment.  Returns a dict: frame_label [T] (-1: nothing left after that frame),
    frame_scores [T, n] (NaN rows where nothing left), eos_label / eos_scores (what left at the end of the stream; -1 / NaN: nothing),
    sum_of_weights, frames_fed, emitted [T] / eos (whether a label left, with or without a winner)."""
    scores = np.asarray(scores, np.float32)
    T, n = scores.shape
    b = Classifier(n, **cfg)
    out = {"frame_label": np.full(T, -1, np.int32), "frame_scores": np.full((T, n), np.nan, np.float32), "eos_label": -1,
           "eos_scores": np.full(n, np.nan, np.float32), "emitted": np.zeros(T, bool), "eos": False}
    t = 0
    while t < T:
        got = b.classify_frame(scores[t], 1.0 if weights is None else weights[t])
        t += 1
        if got is not None:
            out["frame_label"][t - 1], out["frame_scores"][t - 1] = got
            out["emitted"][t - 1] = True
            if b.n_features >= b.n_used:   # !needMoreFeatureVectors(): the rest is read, not scored
                break
    else:
        got = b.classify()
        if got is not None:
            out["eos_label"], out["eos_scores"] = got
            out["eos"] = True
    out["sum_of_weights"], out["frames_fed"] = b.sum_of_weights, t
    return out


def scores_segment(scores, weights=None, delay=INT_MAX, single_frame=False):
    """BayesClassificationScoreNode::work (:429-444) over one segment -> out [T, n] (NaN rows where nothing left), emitted [T] u8,
    eos (0 / 1), eos_out [n]"""
    scores = np.asarray(scores, np.float32)
    T, n = scores.shape
    b = Classifier(n, delay=delay)
    out = {"out": np.full((T, n), np.nan, np.float32), "emitted": np.zeros(T, np.uint8), "eos": 0, "eos_out": np.full(n, np.nan, np.float32)}
    for t in range(T):
        v = b.get_scores_frame(scores[t], 1.0 if weights is None else weights[t])
        if v is not None:
            out["out"][t], out["emitted"][t] = v, 1
            if single_frame:
                b.reset()
    v = b.get_scores()
    if v is not None:
        out["eos"], out["eos_out"] = 1, v
    return out


def is_continuous(cfg):
    d = cfg.get("delay", INT_MAX)
    return cfg.get("window_length", -1) > 0 or 0 <= d < INT_MAX


def classify_batch(scores, frame_offsets, weights=None, **cfg):
    """What amx_bayes_classify_dev leaves in its buffers for a batch: segment_label [n_seg], segment_score [n_seg, n] with `written`
    [n_seg] telling which rows the call writes, frame_label [T_all] (absolute frame index), sum_of_weights [n_seg], and the counter
    (segments, frames) of labels without a winner.
    The segment's label is the one that leaves at the end of the stream, or the single label of segment / first-N mode."""
    scores = np.asarray(scores, np.float32)
    off = np.asarray(frame_offsets, np.int64)
    n_seg, n = len(off) - 1, scores.shape[1]
    res = {"segment_label": np.full(n_seg, -1, np.int32), "segment_score": np.full((n_seg, n), np.nan, np.float32),
           "written": np.zeros(n_seg, bool), "frame_label": np.full(len(scores), -1, np.int32), "sum_of_weights": np.zeros(n_seg, np.float32)}
    no_seg = no_frame = 0
    cont = is_continuous(cfg)
    for s in range(n_seg):
        a, e = int(off[s]), int(off[s + 1])
        r = classify_segment(scores[a:e], None if weights is None else weights[a:e], **cfg)
        res["sum_of_weights"][s] = r["sum_of_weights"]
        emitted = r["emitted"]
        if cont:
            res["frame_label"][a:e] = r["frame_label"]
            no_frame += int(np.sum(emitted & (r["frame_label"] < 0)))
            label, sc, have = r["eos_label"], r["eos_scores"], r["eos"]
        elif emitted.any():   # first N frames
            t = int(np.nonzero(emitted)[0][0])
            label, sc, have = r["frame_label"][t], r["frame_scores"][t], True
        else:
            label, sc, have = r["eos_label"], r["eos_scores"], r["eos"]
        if have:
            res["segment_label"][s], res["segment_score"][s], res["written"][s] = label, sc, True
            no_seg += int(label < 0)
    res["no_winner"] = (no_seg, no_frame)
    return res


def scores_batch(scores, frame_offsets, weights=None, delay=INT_MAX, single_frame=False):
    """What amx_bayes_scores_dev writes: out [T_all, n] (NaN: rows the call leaves alone) and emitted [T_all] (1: the vector left after
    that frame, 2: it left at the end of the stream and is stored in the row of the segment's last frame, 0: nothing)"""
    scores = np.asarray(scores, np.float32)
    off = np.asarray(frame_offsets, np.int64)
    out = np.full(scores.shape, np.nan, np.float32)
    em = np.zeros(len(scores), np.uint8)
    for s in range(len(off) - 1):
        a, e = int(off[s]), int(off[s + 1])
        r = scores_segment(scores[a:e], None if weights is None else weights[a:e], delay, single_frame)
        out[a:e], em[a:e] = r["out"], r["emitted"]
        if r["eos"]:
            out[e - 1], em[e - 1] = r["eos_out"], 2
    return out, em


def pairwise_sum(column):
    """a tree-shaped f32 sum (NOT the reference): what the order test holds the sequential sum against"""
    v = np.asarray(column, np.float32)
    while len(v) > 1:
        if len(v) % 2:
            v = np.concatenate([v, np.zeros(1, np.float32)])
        v = (v[0::2] + v[1::2]).astype(np.float32)
    return v[0] if len(v) else np.float32(0)
