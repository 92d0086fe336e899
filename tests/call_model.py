"""The call-sequence contract of the C ABI (include/sift_mi.h "Call sequence",
sift-features_amd/csrc/result_state.h), restated: given a list of calls, each
marked "ok", "bad" (refused for its arguments) or "late" (fails after a buffer
was touched), the return-code class of every call and the state after it.

A call is (name, outcome, arg): arg is True / False "ran as one chunk" for the
extractions and the new setting for set_keep.  `rows` of a successful producing
call is its position + 1, so a stale count shows which call it came from.
A helper module, not a conftest.
"""
import collections
import itertools

State = collections.namedtuple("State", "where n pyramid batch_readback keep")
START = State("none", 0, False, False, False)
OK, ESTATE, EINVAL, FAILED = "OK", "ESTATE", "EINVAL", "FAILED"
CLEARED = dict(where="none", n=0, pyramid=False, batch_readback=False)
PRODUCING = ("extract", "extract_device", "precompute", "with_precomputed")
NEEDS = {"with_precomputed": lambda s: s.pyramid, "fetch": lambda s: s.where == "host",
         "device_results": lambda s: s.where == "device", "read_pyramid": lambda s: s.pyramid,
         "read_batch": lambda s: s.batch_readback}

# one letter per (call, outcome, arg): the alphabet of the enumeration and the
# text the stand-alone program reads (tests/host_result_state_main.cpp)
ALPHABET = {
    "a": ("extract", "ok", True), "b": ("extract", "ok", False), "c": ("extract", "bad", True),
    "d": ("extract", "late", True),
    "e": ("extract_device", "ok", True), "f": ("extract_device", "ok", False), "g": ("extract_device", "bad", True),
    "h": ("extract_device", "late", True),
    "p": ("precompute", "ok", None), "q": ("precompute", "bad", None), "r": ("precompute", "late", None),
    "s": ("with_precomputed", "ok", None), "t": ("with_precomputed", "bad", None),
    "u": ("with_precomputed", "late", None),
    "F": ("fetch", "ok", None), "D": ("device_results", "ok", None), "P": ("read_pyramid", "ok", None),
    "B": ("read_batch", "ok", None), "k": ("set_keep", "ok", False), "K": ("set_keep", "ok", True),
    "M": ("set_max_octaves", "ok", None),
}


def step(s, call, rows):
    """(return-code class, rows handed out or None, state after) of one call."""
    name, outcome, arg = call
    if name in NEEDS and not NEEDS[name](s):
        return ESTATE, None, s
    if name in PRODUCING and outcome == "bad":
        return EINVAL, None, s
    if name in PRODUCING and outcome == "late":
        return FAILED, None, s._replace(**CLEARED)
    if name in ("extract", "extract_device"):
        where = "device" if name == "extract_device" and s.keep else "host"
        return OK, None, s._replace(where=where, n=rows, pyramid=False, batch_readback=bool(arg))
    if name == "precompute":
        return OK, None, s._replace(where="none", n=0, pyramid=True, batch_readback=False)
    if name == "with_precomputed":
        return OK, None, s._replace(where="host", n=rows, batch_readback=False)
    if name == "set_keep":
        return OK, None, s._replace(keep=bool(arg))
    if name == "set_max_octaves":
        return OK, None, s._replace(pyramid=False, batch_readback=False)
    return OK, (s.n if name in ("fetch", "device_results") else None), s  # the reads


def run(calls, state=START):
    """[(class, rows handed out, state after)] of a list of calls."""
    out = []
    for i, call in enumerate(calls):
        cls, n, state = step(state, call, i + 1)
        out.append((cls, n, state))
    return out


def line(word):
    """The stand-alone program's output line for a word over ALPHABET."""
    res = run([ALPHABET[ch] for ch in word])
    codes = ",".join({OK: "0", ESTATE: "S", EINVAL: "V", FAILED: "L"}[c] + ("" if n is None else f":{n}")
                     for c, n, _ in res)
    s = res[-1][2] if res else START
    return f"{word} {codes} {s.where} {s.n} {int(s.pyramid)}{int(s.batch_readback)}{int(s.keep)}"


def words(max_len):
    """Every word of 1..max_len letters."""
    for k in range(1, max_len + 1):
        for w in itertools.product(ALPHABET, repeat=k):
            yield "".join(w)
