"""The compiled reference (oracle/_ref) where it exists, its recorded answers where it does not.

A few tests hold the oracle to the reference compiled from its own sources, on seeded inputs.  That library is built only where the
reference tree is mounted.  Everywhere else those tests replay the answers it gave to the very same calls:
tests/golden/make_live_golden.py runs each such test once against a Recorder and stores every call in tests/golden/ref_live.npz.
A Replay hands the calls back in order.  Before it answers one, it checks the function name and a digest of every input
(arrays, buffers, scalars), so a test whose inputs drift fails instead of comparing against an answer to another question.

Arguments a test may pass: numpy arrays (or their `.ctypes` object, for void* parameters), ctypes string buffers, `ctypes.byref` of
a ctypes scalar, bytes, numbers, None.  Outputs are the bytes that the call changed in those; the return value is kept exactly.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_live.npz")


def _target(a):
    """the mutable memory behind an argument as a writable uint8 view, or None for an immutable / pointer-free argument"""
    arr = a if isinstance(a, np.ndarray) else getattr(a, "_arr", None)   # an array, or its .ctypes passed for a void* parameter
    if isinstance(arr, np.ndarray):
        if not arr.flags.c_contiguous:
            raise ValueError("a reference call takes C-contiguous arrays")
        return arr.reshape(-1).view(np.uint8)
    obj = getattr(a, "_obj", a)                          # ctypes.byref(x) -> x
    if isinstance(obj, C.Array) and obj._type_ in (C.c_char_p, C.c_wchar_p, C.c_void_p):
        return None
    if isinstance(obj, (C.Array, C._SimpleCData)) and not isinstance(obj, (C.c_char_p, C.c_wchar_p, C.c_void_p)):
        return np.frombuffer((C.c_ubyte * C.sizeof(obj)).from_buffer(obj), np.uint8)
    return None


def _digest(name, args):
    """32 bits of a SHA-1 over the function name and every input: enough to catch inputs that drifted, small enough to store per call"""
    h = hashlib.sha1(name.encode())
    for a in args:
        t = _target(a)
        if t is not None:
            h.update(b"m%d:" % t.size)
            h.update(t.tobytes())
        elif isinstance(a, bytes):
            h.update(b"b" + a)
        elif isinstance(a, C.Array):                     # an array of C strings (names, values)
            h.update(repr(list(a)).encode())
        elif isinstance(a, float):
            h.update(b"f" + float(a).hex().encode())
        else:
            h.update(("r" + repr(a)).encode())
    return int.from_bytes(h.digest()[:4], "little")


class _Recorded:
    """one function of the compiled reference: calls go through and are written down; argtypes / restype reach the real function"""

    def __init__(self, fn, name, rec):
        self.__dict__.update(_fn=fn, _name=name, _rec=rec)

    def __setattr__(self, k, v):
        setattr(self._fn, k, v)

    def __call__(self, *args):
        rec, name = self._rec, self._name
        before = [None if t is None else t.copy() for t in map(_target, args)]
        digest = _digest(name, args)
        ret = self._fn(*args)
        outs = []
        for i, (a, b) in enumerate(zip(args, before)):
            if b is None:
                continue
            diff = np.flatnonzero(_target(a) != b)
            if len(diff):
                lo, hi = int(diff[0]), int(diff[-1]) + 1
                outs.append([i, lo, len(rec.blobs)])
                rec.blobs.append(_target(a)[lo:hi].copy())
        rec.calls.append({"fn": name, "digest": digest, "ret": ret, "outs": outs})
        return ret


class Recorder:
    """wraps the compiled reference; every call goes through and is written down"""

    def __init__(self, lib):
        self._lib, self.calls, self.blobs = lib, [], []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        return _Recorded(fn, name, self) if callable(fn) else fn


class Replay:
    """the recorded calls of one test, answered in the order they were made"""

    def __init__(self, key):
        z = np.load(GOLD, allow_pickle=False)
        meta = json.loads(str(z["meta"]))
        if key not in meta["tests"]:
            raise KeyError("%s holds no recording for %s (tests/golden/make_live_golden.py)" % (GOLD, key))
        self._key, self._names = key, meta["functions"]
        self._first, end = meta["tests"][key]
        self._z = {k: z[k] for k in z.files if k not in ("meta", "pool_planes")}
        self._z["pool"] = np.ascontiguousarray(z["pool_planes"].T).reshape(-1)
        self._next, self._end = self._first, end
        self._outs = np.concatenate([[0], np.cumsum(self._z["n_outs"], dtype=np.int64)])   # call n's outputs: rows _outs[n] .. _outs[n + 1]
        self._used = {self._names[f] for f in self._z["fn"][self._first:end]}

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._used:
            raise AttributeError(name)

        def call(*args):
            z, n = self._z, self._next
            assert n < self._end, "%s: more calls than recorded (next: %s)" % (self._key, name)
            got = self._names[z["fn"][n]]
            assert got == name, "%s: call %d is %s, recorded %s" % (self._key, n - self._first, name, got)
            assert _digest(name, args) == z["digest"][n], "%s: call %d (%s) has other inputs than the recorded one" % (self._key, n - self._first, name)
            self._next += 1
            for j in range(self._outs[n], self._outs[n + 1]):
                b = z["out_blob"][j]
                off, ln = int(z["blob_off"][b]), int(z["blob_len"][b])
                lo = int(z["out_lo"][j])
                _target(args[int(z["out_arg"][j])])[lo:lo + ln] = z["pool"][off:off + ln]
            kind, v = int(z["ret_kind"][n]), z["ret"][n]
            return None if kind == 0 else int(v) if kind == 1 else float(v)
        return call

    def finish(self):
        assert self._next == self._end, "%s: %d of %d recorded calls made" % (self._key, self._next - self._first, self._end - self._first)


def reference(monkeypatch, key, contract="off"):
    """the compiled reference of build `contract` when oracle/_ref holds it (or can build it), else the Replay of test `key`; the
    Replay also answers the oracle.binding helpers (ref_cache_block, ref_accumulate_vector, ...) for the rest of the test"""
    from oracle import binding
    R = binding.load_ref(contract)
    if R is not None:
        return R
    R = Replay(key)
    monkeypatch.setitem(binding._refs, contract, R)
    return R


def finish(R):
    """a replayed test must have made every recorded call"""
    if isinstance(R, Replay):
        R.finish()


def save(recordings):
    """recordings: {key: Recorder} -> tests/golden/ref_live.npz: one row per call (function, input digest, return value, its outputs),
    the output bytes in one pool in which equal outputs are stored once (about 0.2 MB for the five tests)"""
    names, tests, cols = [], {}, {k: [] for k in ("fn", "digest", "ret_kind", "ret", "n_outs", "out_arg", "out_lo", "out_blob")}
    blobs, pool, off = {}, [], 0
    blob_off, blob_len = [], []
    for key, rec in recordings.items():
        first = len(cols["fn"])
        for c in rec.calls:
            if c["fn"] not in names:
                names.append(c["fn"])
            r = c["ret"]
            cols["fn"].append(names.index(c["fn"]))
            cols["digest"].append(c["digest"])
            cols["ret_kind"].append(0 if r is None else 1 if isinstance(r, int) else 2)
            cols["ret"].append(0.0 if r is None else float(r))
            if isinstance(r, int):
                assert float(r) == r, r
            cols["n_outs"].append(len(c["outs"]))
            for i, lo, b in c["outs"]:
                data = rec.blobs[b].tobytes()
                if data not in blobs:
                    blobs[data] = len(blob_off)
                    blob_off.append(off)
                    blob_len.append(len(data))
                    pool.append(data)
                    off += len(data)
                cols["out_arg"].append(i)
                cols["out_lo"].append(lo)
                cols["out_blob"].append(blobs[data])
        tests[key] = [first, len(cols["fn"])]
    types = dict(fn=np.uint16, digest=np.uint32, ret_kind=np.uint8, ret=np.float64, n_outs=np.uint8, out_arg=np.uint8, out_lo=np.uint32,
                 out_blob=np.uint32)
    arrays = {k: np.array(v, types[k]) for k, v in cols.items()}
    raw = b"".join(pool)
    raw += b"\0" * (-len(raw) % 4)
    # the pool as four byte planes (byte k of every 4-byte word together): most outputs are f32 / i32 / f64 words, and deflate finds
    # the runs of their sign-exponent and high bytes only when they sit side by side (the file shrinks by a fifth)
    arrays.update(blob_off=np.array(blob_off, np.uint32), blob_len=np.array(blob_len, np.uint32),
                  pool_planes=np.frombuffer(raw, np.uint8).reshape(-1, 4).T.copy())
    np.savez_compressed(GOLD, meta=np.array(json.dumps(dict(functions=names, tests=tests))), **arrays)
