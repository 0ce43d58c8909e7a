#!/usr/bin/env python
"""Record tests/golden/tem_layouts.json: what temx_plan_set_tem decided -- form, the fourteen cuts, every buffer size --
for some forty plans, as the library answered BEFORE that logic moved into pytemdiags_amd/csrc/tem_layout.hpp.
tests/test_tem_layout_host.py holds the header to it.  Needs a GPU; a case is a plan and one or more temx_plan_set_tem
calls, no fields.

The library has to print what it decided.  It is the one named by TEMX_LIB, built from the commit before the move with
the patch below (not committed anywhere else); it appends one line per temx_plan_set_tem to the file TEMX_DUMP_LAYOUT
names: the buffers and cuts before the call (b_*), the inputs, and the buffers and cuts after it (a_*).
    TEMX_LIB=/path/to/that/libtemx.so python tools/record_tem_layouts.py
Run it again only to add cases: it refuses to write when the library answers a recorded case differently.

The patch (pytemdiags_amd/csrc/temx.hip of the parent commit):

  +// layout dump for tools/record_tem_layouts.py (TEMX_DUMP_LAYOUT names the file the lines are appended to)
  +static size_t g_dump_free = 0;
  +static int g_dump_os_rc = -1000;
  +static void dump_layout_state(FILE* f, const char* tag, const temx_plan* pl) {
  +  const struct { const char* n; const DevBuf* b; } bufs[] = {
  +      {"partial", &pl->partial}, {"B4", &pl->B4}, {"B3", &pl->B3}, {"C4", &pl->C4}, {"zb", &pl->zb}, {"Bs", &pl->Bs},
  +      {"csum", &pl->csum}, {"pbuf", &pl->pbuf}, {"Pq", &pl->Pq}, {"Ax", &pl->Ax}, {"Axs", &pl->Axs}, {"osAt", &pl->osAt},
  +      {"osAb", &pl->osAb}, {"rho", &pl->rho}, {"rho0", &pl->rho0}};
  +  for (const auto& b : bufs) fprintf(f, " %s_%s=%zu", tag, b.n, b.b->bytes);
  +  const struct { const char* n; const Split* s; } sps[] = {
  +      {"proj4", &pl->sp_proj4}, {"eddy", &pl->sp_eddy}, {"proj1", &pl->sp_proj1}, {"cproj4", &pl->sp_cproj4},
  +      {"cproj1", &pl->sp_cproj1}, {"ceddy", &pl->sp_ceddy}, {"cflux", &pl->sp_cflux}, {"lflux", &pl->sp_lflux},
  +      {"copw", &pl->sp_copw}, {"os", &pl->sp_os}, {"os_s", &pl->sp_os_s}, {"sproj4", &pl->sp_sproj4},
  +      {"sproj1", &pl->sp_sproj1}, {"seddy", &pl->sp_seddy}};
  +  for (const auto& s : sps) fprintf(f, " %s_sp_%s=%d,%d,%d,%d", tag, s.n, s.s->ndt, s.s->nsplit, s.s->grid, s.s->dpw);
  +}
  +static void dump_layout_inputs(FILE* f, const temx_plan* pl) {
  +  auto env = [](const char* n) { const char* e = getenv(n); return e && e[0] ? e[0] : '-'; };
  +  fprintf(f, " N=%lld nchunk=%lld K=%d K4=%d M=%d num_cu=%d nlev=%d nt=%lld L=%d TBS=%d large=%d weighted=%d qbasis=%d has_crow=%d"
  +             " unfused=%d lcls=%d cls=%d sym=%d cgroups=%lld cbatches=%lld npg=%lld opt_form=%d bin=%d min_groups=%d"
  +             " env_two_pass=%c env_one_pass=%c env_single_sweep=%c",
  +          (long long)pl->N, (long long)pl->nchunk, pl->K, pl->K4, pl->M, pl->num_cu, pl->nlev, (long long)pl->nt, pl->L, pl->TBS,
  +          (int)pl->large, (int)pl->weighted, (int)pl->qbasis, (int)!pl->h_crow.empty(), (int)unfused_stage2(pl), (int)pl->lcls,
  +          (int)pl->cls, (int)pl->sym, (long long)pl->cgroups, (long long)pl->cbatches, (long long)pl->npg, pl->opt_form,
  +          (int)bin_mode(pl), pl->opt_single_sweep_min_groups, env("TEMX_TWO_PASS"), env("TEMX_ONE_PASS"), env("TEMX_SINGLE_SWEEP"));
  +}
  +struct LayoutDump {
  +  FILE* f = nullptr;
  +  const temx_plan* pl;
  +  explicit LayoutDump(const temx_plan* p) : pl(p) {
  +    if (const char* path = getenv("TEMX_DUMP_LAYOUT")) f = fopen(path, "a");
  +    g_dump_free = 0;
  +    g_dump_os_rc = -1000;
  +    if (f) {
  +      fprintf(f, "TEMX_LAYOUT");
  +      dump_layout_state(f, "b", pl);
  +    }
  +  }
  +  void done() {
  +    if (!f) return;
  +    dump_layout_inputs(f, pl);
  +    fprintf(f, " KX=%d KR=%d NQ=%d sbatches=%lld free=%zu os_rc=%d onepass=%d lone=%d os_on=%d", pl->KX, pl->KR, pl->NQ,
  +            (long long)pl->sbatches, g_dump_free, g_dump_os_rc, (int)pl->onepass, (int)pl->lone, (int)pl->os_on);
  +    dump_layout_state(f, "a", pl);
  +    fprintf(f, " ok=1");
  +  }
  +  ~LayoutDump() {
  +    if (f) {
  +      fprintf(f, "\\n");
  +      fclose(f);
  +    }
  +  }
  +};
  +
   int temx_plan_set_tem(temx_plan* pl, int nlev, int64_t nt, const double* p_pa_host, double p0) try {
  ...
     // (tem_ready fails) until the last allocation has succeeded
  +  LayoutDump dump(pl);
     pl->tem = false;
  ...
           pl->pbuf.ensure(need_pb) == TEMX_OK) {
  +      g_dump_free = fr;
         HIPCHK(hipMemset(pl->csum.p, 0, pl->csum.bytes));
  ...
             have = true;
           }
  +        g_dump_free = fr;
           if (have) {
  ...
                 rc = build_os_tables(pl);
  +              g_dump_os_rc = rc;
                 if (rc == TEMX_ERANK) want = false;          // too few distinct latitudes in the subsample: class-sum form
  ...
     if (bin_mode(pl) && (rc = bin_set_tem(pl))) return rc;   // tables (first time) and the workspace of the binned sweeps
  +  dump.done();
     pl->tem = true;

free is what hipMemGetInfo answered where the memory rule was asked (0: not asked), os_rc what build_os_tables answered
(-1000: not called).
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "tem_layouts.json")
ENV = ("TEMX_TWO_PASS", "TEMX_ONE_PASS", "TEMX_SINGLE_SWEEP")

SMALL, LEV, LONG = (7, 3), (30, 2), (72, 30)        # D = 21 (ragged, one d-tile per workgroup), 60, 2160
BELOW, ABOVE = (8, 30), (8, 31)                     # on ne30: 48 602 x 240 = 11 664 480 and x 248 = 12 053 296 around 1.2e7


def case(name, grid, L, *shapes, **kw):
    return dict(name=name, grid=grid, L=L, shapes=list(shapes), **kw)


# a case is one plan and one temx_plan_set_tem per shape (the later ones find the earlier ones' buffers)
CASES = [
    case("ne4_L20_small", "ne4", 20, SMALL), case("ne4_L20_lev", "ne4", 20, LEV), case("ne4_L20_long", "ne4", 20, LONG),
    case("ne4_L50_lev", "ne4", 50, LEV),
    case("ne8_L50_small", "ne8", 50, SMALL), case("ne8_L50_lev", "ne8", 50, LEV), case("ne8_L50_long", "ne8", 50, LONG),
    case("ne8_L20_long", "ne8", 20, LONG),
    case("ne30_L50_below", "ne30", 50, BELOW), case("ne30_L50_above", "ne30", 50, ABOVE), case("ne30_L50_long", "ne30", 50, LONG),
    case("ne30_L20_above", "ne30", 20, ABOVE),
    case("latlon_L20_small", "latlon", 20, SMALL), case("latlon_L20_lev", "latlon", 20, LEV), case("latlon_L50_long", "latlon", 50, LONG),
    # the mirror-paired, the generic and the weighted sweeps
    case("ne8_sym_L20_lev", "ne8", 20, LEV, classes=False), case("ne8_sym_L50_small", "ne8", 50, SMALL, classes=False),
    case("ne8_sym_L50_long", "ne8", 50, LONG, classes=False),
    case("ne8_generic_L20_lev", "ne8", 20, LEV, classes=False, symmetry=False),
    case("ne8_generic_L50_long", "ne8", 50, LONG, classes=False, symmetry=False),
    case("ne4_weights_L20_lev", "ne4", 20, LEV, weights=True), case("ne8_weights_L50_long", "ne8", 50, LONG, weights=True),
    # K > 64: the large-L class path with four d-tiles or more, and below
    case("ne8_L70_long", "ne8", 70, LONG), case("ne8_L70_small", "ne8", 70, SMALL), case("ne8_L70_lev", "ne8", 70, LEV),
    case("ne8_L70_long_two_pass", "ne8", 70, LONG, form=0),
    # eight blocks of even harmonics: the single sweep has no instantiation
    case("ne30_L60_above", "ne30", 60, ABOVE),
    # every TEMX_OPT_FORM value, on a grid the automatic choice sends to the single sweep and on one it leaves two-pass
    *[case("ne30_L50_above_form%d" % f, "ne30", 50, ABOVE, form=f) for f in (0, 1, 2, 3)],
    *[case("ne8_L50_long_form%d" % f, "ne8", 50, LONG, form=f) for f in (0, 1, 2, 3)],
    case("ne4_L50_long_form2", "ne4", 50, LONG, form=2),
    # TEMX_OPT_SINGLE_SWEEP_MIN_GROUPS on both sides of the group count (ne30: 760 class-groups)
    case("ne30_L50_above_min700", "ne30", 50, ABOVE, min_groups=700), case("ne30_L50_above_min800", "ne30", 50, ABOVE, min_groups=800),
    case("ne8_L50_long_form1_min10", "ne8", 50, LONG, env={"TEMX_ONE_PASS": "1"}, min_groups=10),
    case("ne8_L20_lev_bins128", "ne8", 20, LEV, lat_bins=128), case("ne8_L20_lev_missing", "ne8", 20, LEV, missing="mask"),
    # the environment over the options
    case("ne30_L50_above_env_two_pass", "ne30", 50, ABOVE, env={"TEMX_TWO_PASS": "1"}),
    case("ne30_L50_above_env_no_sweep", "ne30", 50, ABOVE, env={"TEMX_SINGLE_SWEEP": "0"}),
    case("ne8_L50_long_env_one_pass", "ne8", 50, LONG, env={"TEMX_ONE_PASS": "1"}),
    case("ne8_L50_long_env_sweep", "ne8", 50, LONG, env={"TEMX_ONE_PASS": "1", "TEMX_SINGLE_SWEEP": "1"}),
    case("ne8_L50_long_form2_env_two_pass", "ne8", 50, LONG, form=2, env={"TEMX_TWO_PASS": "1"}),
    # again on the same plan, shorter and longer: csum and the other buffers are held
    case("ne30_L50_again", "ne30", 50, ABOVE, (8, 20), (8, 40)), case("ne30_L50_held", "ne30", 50, (8, 40), ABOVE, (8, 50)),
    case("ne8_L70_again", "ne8", 70, LONG, (72, 10), (72, 40)),
]


def grid(name):
    from pytemdiags_amd import synth
    if name.startswith("ne"):
        return synth.cubed_sphere_gll(int(name[2:]))[0]
    assert name == "latlon"        # tests/test_host_tables.py: 64 rows x 1440 longitudes and 33 more columns on the equator
    north = (np.arange(32) + 0.5) * (90.0 / 32.5)
    return np.concatenate([np.repeat(np.concatenate([-north[::-1], north]), 1440), np.zeros(33)])


def parse(line):
    """One dumped line -> {key: int, [ints] or str}."""
    rec = {}
    for tok in line.split()[1:]:
        k, v = tok.split("=", 1)
        rec[k] = [int(x) for x in v.split(",")] if "," in v else (int(v) if v.lstrip("-").isdigit() else v)
    return rec


def run_case(c, dump):
    from pytemdiags_amd import engine, synth
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(c.get("env", {}))
    edges = np.arange(-90, 91, 1.0)
    plan = engine.Plan(grid(c["grid"]), (edges[1:] + edges[:-1]) / 2, c["L"], symmetry=c.get("symmetry", True),
                       classes=c.get("classes", True))
    try:
        if c.get("weights"):
            plan.set_weights(np.cos(np.deg2rad(grid(c["grid"]))) + 0.5)
        for key in ("form", "lat_bins", "missing"):
            if key in c:
                plan.configure(**{key: c[key]})
        if "min_groups" in c:
            plan.configure(single_sweep_min_groups=c["min_groups"])
        open(dump, "w").close()
        for nlev, nt in c["shapes"]:
            plan.set_tem(nlev, nt, synth.pressure_levels(nlev) * 100)
    finally:
        plan.close()
        for k in ENV:
            os.environ.pop(k, None)
    recs = [parse(line) for line in open(dump) if line.startswith("TEMX_LAYOUT")]
    assert len(recs) == len(c["shapes"]) and all(r.get("ok") == 1 for r in recs), (c["name"], recs)
    return recs


def main():
    if "TEMX_LIB" not in os.environ:
        sys.exit("TEMX_LIB must name a library built from the commit before the move, with the dump patch (see the docstring)")
    old = {r["name"]: r for r in json.load(open(GOLDEN))["records"]} if os.path.exists(GOLDEN) else {}
    dump = os.path.join(tempfile.mkdtemp(), "layout.txt")
    os.environ["TEMX_DUMP_LAYOUT"] = dump
    rows, failed = [], []
    for c in CASES:
        try:
            recs = run_case(c, dump)
        except Exception as e:          # report every case that does not run, write nothing
            failed.append("%s: %r" % (c["name"], e))
            continue
        for i, rec in enumerate(recs):
            name = "%s/%d" % (c["name"], i)
            row = {"name": name, "v": rec}
            was = old.pop(name, None)
            # (free memory is the one input that is the machine's: a recorded case keeps its own)
            if was is not None:
                if {k: v for k, v in was["v"].items() if k != "free"} != {k: v for k, v in rec.items() if k != "free"}:
                    sys.exit("%s: recorded %r, this library answers %r; nothing written" % (name, was["v"], rec))
                row = was
            rows.append(row)
            v = row["v"]
            print("%-36s onepass=%d lone=%d os_on=%d os_rc=%d partial=%d" % (name, v["onepass"], v["lone"], v["os_on"], v["os_rc"],
                                                                              v["a_partial"]), flush=True)
    if failed:
        sys.exit("nothing written:\n" + "\n".join(failed))
    if old:
        sys.exit("%d recorded cases are no longer generated; nothing written" % len(old))
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as fh:
        fh.write('{\n "count": %d,\n "records": [\n%s\n ]\n}\n' % (len(rows), ",\n".join("  " + json.dumps(r) for r in rows)))
    print("%d records -> %s" % (len(rows), out))


if __name__ == "__main__":
    main()
