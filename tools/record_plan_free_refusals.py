#!/usr/bin/env python
"""Record tests/golden/plan_free_refusals.json: what the four plan-free entry points (temxv_interp, temxl_to_engine,
temxi_records_to_pressure, temxc_time_sum) answer to a few hundred argument sets, each of which breaks one rule or
none.  Every call names device 99 and fake addresses, so it needs no GPU: a refusal is -1 with its message, a call
that got past the checks is -2 (only the code is stored: the text is the HIP runtime's).

The fixture was recorded while the rules still stood four times over in temx.hip; tests/test_field_args_host.py holds
field_args.hpp to it.  Run it again only to add cases.  It refuses to write when the library answers a case that is
already in the fixture differently from what is recorded there (temxv_interp's wording changed on purpose, so that means:
run it against a library built from the commit before the move, through TEMX_LIB):
    TEMX_LIB=/path/to/that/libtemx.so python tools/record_plan_free_refusals.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_field_args_host import GOLDEN, call_case  # noqa: E402

NAN, INF = float("nan"), float("inf")
A, B, D, E, P = 4096, 8192, 1 << 20, 1 << 21, 1 << 24          # src 0, src 1, out 0, out 1, ps

DEFAULTS = {
    "temxv": dict(nf=1, src=[A], dst=[D], dtype=0, ncol=4, nlev=3, nt=2, nplev=2, plev=[5e4, 7e4], pmode=0,
                  hyam=[0.1, 0.2, 0.3], hybm=[0.1, 0.2, 0.3], p0=1e5, ps=P, pdt=0, method=0, edge=0),
    "temxl": dict(nf=1, src=[A], sdt=[0], dst=[D], ddt=0, ncol=4, nlev=3, nt_src=5, t0=1, ntb=2, flags=0),
    "temxi": dict(nf=1, src=[A], sdt=[0], dst=[D], ddt=0, ncol=4, nlev=3, nt_src=5, t0=1, ntb=2, nplev=2,
                  plev=[5e4, 7e4], hyam=[0.1, 0.2, 0.3], hybm=[0.1, 0.2, 0.3], p0=1e5, ps=P, pdt=0, method=0, edge=0),
    "temxc": dict(nf=1, src=[A], sdt=[0], acc=[D], ncol=4, nlev=3, nt=5, flags=0),
}
# bytes of one fp64 source and of one output at the default sizes, the name of the outputs and of the record length
SHAPE = {"temxv": (192, 128, "dst", "nt"), "temxl": (480, 192, "dst", "nt_src"), "temxi": (480, 128, "dst", "nt_src"),
         "temxc": (480, 96, "acc", "nt")}


def field_cases(fn):
    """The rules on nf, the pointer arrays, sizes and aliasing, which all four entry points have."""
    sb, ob, out, nt = SHAPE[fn]
    per_field = fn != "temxv"                          # temxv_interp has one dtype for all fields
    two = dict(nf=2, src=[A, B], **{out: [D, E]})
    three = dict(nf=3, src=[A, B, 3 * A], **{out: [D, E, 3 * D]})
    if per_field:
        two["sdt"], three["sdt"] = [0, 0], [0, 0, 0]
    c = [dict(), dict(two), dict(three), dict(nf=0), dict(nf=9), dict(nf=-1), dict(src=None), {out: None},
         dict(src=[None]), {out: [None]}, dict(two, src=[A, None]), dict(two, **{out: [D, None]}),
         dict(two, src=[None, B]), dict(three, **{out: [D, E, None]}),
         dict(ncol=0), dict(nlev=0), {nt: 0}, dict(ncol=-1), dict(nlev=1), dict(nlev=2),
         dict(nlev=(1 << 20) + 1), {nt: (1 << 31) + 1}, dict(ncol=(1 << 40) + 1),
         # fp64 at 4 mod 8
         dict(src=[A + 4]), {out: [D + 4]}, dict(two, src=[A, B + 4]), dict(two, **{out: [D, E + 4]}),
         # an output against a source: the same, inside, one element at either end, touching at either end
         {out: [A]}, {out: [A + 64]}, {out: [A + 8]}, {out: [A + sb - 8]}, {out: [A - ob + 8]}, {out: [A + sb]},
         {out: [A - ob]},
         dict(two, **{out: [D, A + 8]}), dict(two, **{out: [B + 8, D]}), dict(two, **{out: [D, B + 8]}),
         dict(two, **{out: [D, B + sb]}), dict(two, **{out: [B - ob, D]}),
         dict(three, **{out: [D, E, A + 16]}), dict(three, **{out: [D, E, 3 * A + sb - 8]}),
         # an output against an earlier output
         dict(two, **{out: [D, D]}), dict(two, **{out: [D, D + ob - 8]}), dict(two, **{out: [D + 8, D]}),
         dict(two, **{out: [D, D + ob]}), dict(two, **{out: [D + ob, D]}),
         dict(three, **{out: [D, E, E + 8]}), dict(three, **{out: [D, E, D + ob - 8]}), dict(three, **{out: [D, E, E + ob]})]
    if fn != "temxv":                                  # its product of sizes had no cap when this was recorded
        c += [dict(ncol=1 << 40, nlev=1 << 20), {"ncol": 1 << 40, nt: 1 << 31}, {"nlev": 1 << 20, nt: 1 << 31, "ncol": 1 << 10}]
    if per_field:
        c += [dict(sdt=None), dict(sdt=[2]), dict(sdt=[7]), dict(sdt=[-1]), dict(two, sdt=[0, 7]), dict(three, sdt=[1, 0, 3]),
              dict(sdt=[1]), dict(two, sdt=[0, 1]), dict(two, sdt=[1, 0]),
              # fp32 sources: aligned to 4, and half as long
              dict(src=[A + 4], sdt=[1]), dict(src=[A + 2], sdt=[1]), dict(two, src=[A, B + 2], sdt=[0, 1]),
              dict(two, src=[A, B + 4], sdt=[0, 1]),
              dict(sdt=[1], **{out: [A + sb // 2]}), dict(sdt=[1], **{out: [A + sb // 2 - 8]}),
              dict(two, sdt=[0, 1], **{out: [D, B + sb // 2]}), dict(two, sdt=[0, 1], **{out: [D, B + sb // 2 - 8]}),
              dict(two, sdt=[1, 0], **{out: [D, B + sb // 2]})]
    return c


def window_cases():
    """temxl_to_engine and temxi_records_to_pressure: the window t0 .. t0 + ntb of nt_src, and the dtype of dst."""
    two = dict(nf=2, src=[A, B], sdt=[0, 0], dst=[D, E])
    return [dict(ntb=0), dict(ntb=-2), dict(t0=-1), dict(t0=4), dict(t0=0, ntb=6), dict(t0=5, ntb=1), dict(t0=1 << 62),
            dict(t0=3), dict(t0=0, ntb=5), dict(t0=4, ntb=1), dict(t0=0), dict(nt_src=1, t0=0, ntb=1),
            dict(ddt=2), dict(ddt=5), dict(ddt=-1), dict(ddt=1), dict(two, sdt=[1, 0], ddt=1), dict(two, sdt=[0, 1], ddt=1),
            dict(sdt=[1], ddt=1), dict(two, sdt=[1, 1], ddt=1), dict(sdt=[1], ddt=1, dst=[D + 4]),
            dict(sdt=[1], ddt=1, dst=[D + 2]), dict(ddt=1, sdt=[1], src=[A + 4])]


def level_cases(fn):
    """temxv_interp and temxi_records_to_pressure: the target levels, the hybrid coefficients and the pressure input."""
    ps_bytes = 64 if fn == "temxv" else 160            # ps [ncol][nt] and [ncol][nt_src], fp64
    ob = SHAPE[fn][1]
    hy4 = [0.0, 0.1, 0.2, 0.3]
    return [dict(plev=None), dict(hyam=None), dict(hybm=None), dict(ps=None), dict(pdt=2), dict(pdt=-1),
            dict(method=2), dict(method=-1), dict(method=1), dict(edge=-1), dict(edge=2), dict(edge=1),
            dict(nplev=0), dict(nplev=-1), dict(nplev=(1 << 20) + 1), dict(nplev=1, plev=[5e4]),
            dict(nplev=3, plev=[1e3, 5e4, 7e4]), dict(nlev=4, hyam=hy4, hybm=hy4), dict(nlev=2, hyam=[0.1, 0.2], hybm=[0.0, 0.5]),
            dict(p0=NAN), dict(p0=INF), dict(p0=-INF), dict(p0=0.0), dict(p0=-1e5),
            dict(plev=[7e4, 5e4]), dict(plev=[5e4, 5e4]), dict(plev=[-1.0, 5e4]), dict(plev=[0.0, 5e4]), dict(plev=[5e4, INF]),
            dict(plev=[NAN, 5e4]), dict(plev=[5e4, NAN]), dict(nplev=3, plev=[1e3, 5e4, 4e4]), dict(nplev=3, plev=[1e3, -5e4, 7e4]),
            dict(hyam=[0.1, NAN, 0.3]), dict(hybm=[0.1, 0.2, INF]), dict(hyam=[-INF, 0.2, 0.3]), dict(hybm=[NAN, 0.2, 0.3]),
            dict(hyam=[0.3, 0.2, 0.1]), dict(hybm=[-0.1, 0.0, 0.0]),
            dict(ps=P + 4), dict(ps=P + 2, pdt=1), dict(ps=P + 4, pdt=1), dict(pdt=1),
            dict(dst=[P]), dict(dst=[P + 8]), dict(dst=[P + ps_bytes - 8]), dict(dst=[P - ob + 8]), dict(dst=[P + ps_bytes]),
            dict(dst=[P - ob]), dict(pdt=1, dst=[P + ps_bytes // 2]), dict(pdt=1, dst=[P + ps_bytes // 2 - 8]),
            dict(nf=2, src=[A, B], dst=[D, P + 8], **({} if fn == "temxv" else {"sdt": [0, 0]}))]


def cases(fn):
    c = field_cases(fn)
    if fn in ("temxl", "temxc"):
        c += [dict(flags=1), dict(flags=2), dict(flags=-1), dict(flags=4), dict(flags=3)]
    if fn in ("temxl", "temxi"):
        c += window_cases()
    if fn in ("temxv", "temxi"):
        c += level_cases(fn)
    if fn == "temxl":          # the refusal list of tests/test_gpu_layout.py, with fake addresses in place of tensors
        s, h, n = [1 << 16, 1 << 17], [1 << 22, 1 << 23], 40 * 3 * 4
        good = dict(nf=2, src=s, sdt=[0, 0], dst=h, ddt=0, ncol=40, nlev=3, nt_src=9, t0=2, ntb=4, flags=0)
        c += [dict(good, **kw) for kw in (
            dict(), dict(flags=1), dict(nf=0), dict(nf=9), dict(src=None), dict(sdt=None), dict(dst=None), dict(src=[s[0], None]),
            dict(dst=[None, h[1]]), dict(ncol=0), dict(nlev=0), dict(nt_src=0), dict(ntb=0), dict(t0=-1), dict(t0=6),
            dict(ntb=10, t0=0), dict(flags=2), dict(flags=-1), dict(sdt=[0, 7]), dict(ddt=5), dict(ddt=1),
            dict(src=[s[0] + 4, s[1]]), dict(src=[s[0], s[1] + 2], sdt=[0, 1]), dict(dst=[h[0], h[1] + 4]),
            dict(dst=[s[1] + 8 * 5, h[1]]), dict(dst=[h[0], s[0] + 8 * (9 * 3 * 40 - 1)]), dict(dst=[h[0], h[0] + 8 * (n - 1)]))]
        # the refusals that depend on the tile come after every argument check and before the device
        far = dict(src=[1 << 60], dst=[1 << 50])
        c += [dict(far, ncol=(1 << 35) + 1, nlev=1, nt_src=1, t0=0, ntb=1), dict(far, ncol=1 << 35, nlev=1, nt_src=1, t0=0, ntb=1),
              dict(far, ncol=1 << 40, nlev=1 << 8, nt_src=1, t0=0, ntb=1)]
    if fn == "temxi":
        far = dict(src=[1 << 60], dst=[1 << 50], ps=1 << 56)
        c += [dict(far, ncol=(1 << 34) + 1), dict(far, ncol=1 << 34), dict(ncol=1 << 40, nplev=1 << 20),
              dict(sdt=[1], ddt=1, pdt=1, method=1, edge=1), dict(nf=2, src=[A, B], sdt=[0, 0], dst=[D, D + 16]),
              dict(nlev=2, plev=[5e4], nplev=1, hyam=[0.1, 0.2], hybm=[0.0, 0.5])]
    if fn == "temxc":
        c += [dict(src=[1 << 60], acc=[1 << 52], ncol=1 << 40, nlev=1 << 8, nt=1), dict(nt=1), dict(nt=2000),
              dict(nf=2, src=[A, B], sdt=[0, 1], acc=[D, D + 88]), dict(nf=2, src=[A, B], sdt=[0, 1], acc=[D, D + 96])]
    if fn == "temxv":
        # field mode: hyam, hybm and p0 are not read, and the pressure input is as long as a source of p_dtype
        c += [dict(pmode=2), dict(pmode=-1), dict(pmode=1), dict(pmode=1, hyam=None, hybm=None), dict(pmode=1, p0=NAN),
              dict(pmode=1, hyam=[NAN, 0.2, 0.3]), dict(pmode=1, dst=[P + 64]), dict(pmode=1, dst=[P + 184]),
              dict(pmode=1, dst=[P + 192]), dict(pmode=1, pdt=1, dst=[P + 96]), dict(pmode=1, pdt=1, dst=[P + 88]),
              dict(dtype=2), dict(dtype=-1), dict(dtype=1), dict(dtype=1, src=[A + 4], dst=[D + 4]), dict(dtype=1, src=[A + 2]),
              dict(dtype=1, dst=[D + 2]), dict(dtype=1, dst=[A + 96]), dict(dtype=1, dst=[A + 88]), dict(dtype=1, dst=[A - 64]),
              dict(dtype=1, dst=[A - 56])]
    return c


def main():
    out = {"defaults": DEFAULTS, "cases": {}, "count": {}}
    old = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"defaults": DEFAULTS, "cases": {}}
    for fn in ("temxv", "temxl", "temxi", "temxc"):
        if old["defaults"][fn] != json.loads(json.dumps(DEFAULTS[fn])):
            sys.exit("%s: the defaults differ from the fixture's; its cases would mean something else" % fn)
        known = {json.dumps(r["args"], sort_keys=True): r for r in old["cases"].get(fn, [])}
        rows = []
        for args in cases(fn):
            rc, msg = call_case(fn, args, DEFAULTS[fn])
            assert rc < 0, (fn, args, rc, msg)       # device 99: no call can succeed
            rows.append({"args": args, "rc": rc} if rc == -2 else {"args": args, "rc": rc, "msg": msg})
            was = known.pop(json.dumps(args, sort_keys=True), None)
            if was is not None and (was["rc"], was.get("msg")) != (rows[-1]["rc"], rows[-1].get("msg")):
                sys.exit("%s %r: recorded %r, this library answers %r; nothing written" % (fn, args, was, rows[-1]))
        if known:
            sys.exit("%s: %d recorded cases are no longer generated; nothing written" % (fn, len(known)))
        out["cases"][fn], out["count"][fn] = rows, len(rows)
        print("%s: %d cases, %d refused, %d reached the device" % (fn, len(rows), sum(r["rc"] != -2 for r in rows),
                                                                  sum(r["rc"] == -2 for r in rows)))
    with open(GOLDEN, "w") as fh:
        fh.write("{\n")
        fh.write(' "defaults": {\n%s\n },\n' % ",\n".join('  "%s": %s' % (k, json.dumps(v)) for k, v in out["defaults"].items()))
        fh.write(' "count": %s,\n "cases": {\n' % json.dumps(out["count"]))
        fh.write(",\n".join('  "%s": [\n%s\n  ]' % (fn, ",\n".join("   " + json.dumps(r) for r in rows))
                            for fn, rows in out["cases"].items()))
        fh.write("\n }\n}\n")


if __name__ == "__main__":
    main()
