"""The reference writer of trace files, in pure Python: pretty(x), the text of a float32 widened to float64 as serde_json / ryu
print it, from the shortest digits Python's repr gives, and trace_text(trace), the bytes of a trace file (csrc/trace_json.hpp) for
a dict in SelfPlay.trace's shape, with the optional "fen" and "opening" members.  Also the float bit patterns the tests share."""
import math

import numpy as np

FRACTIONS = (0, 1, 0x400000, 0x7FFFFF, 0x2AAAAA)   # of every exponent


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def edge_bits(signs=(0, 1)):
    """every exponent x FRACTIONS x signs, the patterns around the layout boundaries 1e-5 / 1e16 / 1e17 (and 1e-4, 1e15, 1, the
    largest and the smallest normal), the zeros, infinities and a NaN -> uint32 array"""
    out = [(s << 31) | (e << 23) | f for e in range(256) for f in FRACTIONS for s in signs]
    for v in (1e-5, 1e-4, 1e15, 1e16, 1e17, 1.0, 3.4028235e38, 1.1754944e-38):
        b = int(np.float32(v).view(np.uint32))
        out += [b + d for d in range(-3, 4)]
    out += [0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000]
    return np.array(out, np.uint32)


def pretty(x):
    """the text of float32 x, widened to float64, in ryu's pretty layout: the five cases of fmt_f64 (csrc/trace_json.hpp)"""
    v = float(np.float32(x))
    if math.isnan(v) or math.isinf(v):
        return "null"
    if v == 0.0:
        return "-0.0" if math.copysign(1.0, v) < 0 else "0.0"
    mant, _, e = repr(abs(v)).partition("e")
    ip, _, fp = mant.partition(".")
    k = (int(e) if e else 0) - len(fp)      # value = int(ip + fp) * 10^k
    digits = (ip + fp).lstrip("0")
    k += len(digits) - len(digits.rstrip("0"))
    digits = digits.rstrip("0")
    kk = k + len(digits)                    # value = 0.digits * 10^kk
    if 0 <= k and kk <= 16:
        body = digits + "0" * k + ".0"
    elif 0 < kk <= 16:
        body = digits[:kk] + "." + digits[kk:]
    elif -5 < kk <= 0:
        body = "0." + "0" * -kk + digits
    elif len(digits) == 1:
        body = f"{digits}e{kk - 1}"
    else:
        body = f"{digits[0]}.{digits[1:]}e{kk - 1}"
    return ("-" if v < 0 else "") + body


def trace_text(trace):
    """the bytes sctrace::trace_to_json writes for the trace"""
    o = ['{\n  "outcome": ']
    oc = trace.get("outcome")
    if oc is None:
        o.append("null")
    else:
        w = oc["winner"]
        o.append('{\n    "termination": "%s",\n    "winner": %s\n  }' % (oc["termination"], "null" if w is None else f'"{w}"'))
    o.append(',\n  "steps": ')
    steps = trace["steps"]
    if not steps:
        o.append("[]")
    else:
        o.append("[\n")
        for i, (mv, q, children) in enumerate(steps):
            o.append(f'    [\n      "{mv}",\n      {pretty(q)},\n      ')
            if not children:
                o.append("[]")
            else:
                o.append("[\n")
                for c, (cm, cn, cq, cu) in enumerate(children):
                    o.append(f'        [\n          "{cm}",\n          {int(cn)},\n          {pretty(cq)},\n          {pretty(cu)}\n        ]')
                    o.append(",\n" if c + 1 < len(children) else "\n")
                o.append("      ]")
            o.append("\n    ]")
            o.append(",\n" if i + 1 < len(steps) else "\n")
        o.append("  ]")
    if trace.get("fen"):
        o.append(',\n  "fen": "%s"' % trace["fen"])
    if trace.get("opening"):
        o.append(',\n  "opening": [\n')
        o.append(",\n".join(f'    "{m}"' for m in trace["opening"]))
        o.append("\n  ]")
    o.append("\n}")
    return "".join(o).encode()
