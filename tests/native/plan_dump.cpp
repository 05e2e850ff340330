// The host plans of the MSM and accumulator drivers and of the pairing decider
// (msm_plan.hpp, accum_plan.hpp, pairing_plan.hpp) as text, for
// tests/test_plan_native.py and tests/pairing_lazy_model.py: g++ -O2 -std=c++17,
// no HIP.  One query per line on stdin, one line of key=value fields per
// query on stdout (lists as comma-separated values):
//   consts
//   msm n c min_chunk                       make_plan
//   parts n fixed host split                msm_parts
//   sort n c min_chunk fixed rows host split cache_kb chunk_kb
//                                           msm_schedule: every part's sort plan (a table: window c, rows
//                                           merged rows, rows padded to kSortB) as pK_key=value
//   reduce n c min_chunk fixed rows         reduce_plan
//   small n                                 small_plan
//   many n                                  many_pick_c and its windows / bytes per base
//   manyc c                                 many_windows, many_bytes_per_base
//   manykq total                            many_kq
//   acc B T Tp npair split tpl ladder [nvk_build row_bytes tail_bytes lds_cap]
//                                           acc_path
//   terms nfixed nperm qdeg p_h p_W nsets { len { kind idx eval } * len } * nsets
//                                           acc_terms of the rotation sets given as (ref kind, ref index, eval)
//   pairing                                 pairing_plan.hpp: the program's words (prog), step_doubles of every
//                                           step (doubles), kFrob as 2 x 6 x 2 x 4 words (frob) and the geometry
// An unknown query prints "error=..." and the program exits with status 2.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../halo2-aggregation_amd/csrc/accum_plan.hpp"
#include "../../halo2-aggregation_amd/csrc/msm_plan.hpp"
#include "../../halo2-aggregation_amd/csrc/pairing_plan.hpp"

using namespace pm;

static void kv(const char* k, unsigned long long v) { std::printf("%s=%llu ", k, v); }
static void kvs(const std::string& k, unsigned long long v) { std::printf("%s=%llu ", k.c_str(), v); }
static void list(const char* k, const std::vector<uint32_t>& v) {
  std::printf("%s=", k);
  for (size_t i = 0; i < v.size(); i++) std::printf(i ? ",%u" : "%u", v[i]);
  std::printf(" ");
}

static void consts() {
  kv("kMinC", kMinC), kv("kMaxC", kMaxC), kv("kAutoMaxC", kAutoMaxC), kv("kL1", kL1);
  kv("kSortThreads", kSortThreads), kv("kSortPerThread", kSortPerThread), kv("kSortB", kSortB);
  kv("kFineThreads", kFineThreads), kv("kFineChunkBytes", kFineChunkBytes), kv("kMaxLds", kMaxLds);
  kv("kScanThreads", kScanThreads), kv("kScanPerThread", kScanPerThread), kv("kScanChunk", kScanChunk);
  kv("kMaxParts", kMaxParts), kv("kSplitCopyMinN", kSplitCopyMinN), kv("kSplitCopy3MinN", kSplitCopy3MinN);
  kv("kTJobs", kTJobs), kv("kMaxSplit", kMaxSplit), kv("kBitsSplitK", kBitsSplitK), kv("kRedThreads", kRedThreads);
  kv("kSmallWin", kSmallWin), kv("kSmallQuads", kSmallQuads), kv("kSmallFusedN", kSmallFusedN);
  kv("kSmallSlices", kSmallSlices), kv("kSmallLanesT", kSmallLanesT);
  kv("kManyQuads", kManyQuads), kv("kManyQuadBudget", kManyQuadBudget), kv("kManyTabBudget", kManyTabBudget);
  kv("kManyTabCap", kManyTabCap);
  kv("kAccLaneBudget", kAccLaneBudget), kv("kAccSumLanes", kAccSumLanes), kv("kAccSlicedChains", kAccSlicedChains);
}

static void dump_plan(const MsmPlan& p) {
  kv("c", p.c), kv("W", p.W), kv("base", p.base), kv("extra", p.extra), kv("cmax", p.cmax), kv("K", p.K);
  kv("L1", p.L1), kv("log2L1", p.log2L1), kv("NB", p.NB), kv("M1", p.M1), kv("NB2", p.NB2), kv("n", p.n);
  kv("chunk", p.chunk), kv("nthreads", p.nthreads);
}

static void dump_geom(const std::string& pre, const SortGeom& g) {
  kvs(pre + "FB", g.FB), kvs(pre + "NCB", g.NCB), kvs(pre + "nblk", g.nblk), kvs(pre + "blk0", g.blk0);
  kvs(pre + "ppt", g.ppt), kvs(pre + "hsub", g.hsub), kvs(pre + "rstride", g.rstride);
  kvs(pre + "rdelta", g.rdelta), kvs(pre + "roff", g.roff);
}

static void dump_reduce(const ReducePlan& r) {
  kv("Wr", r.Wr), kv("TOT", r.TOT), kv("NJ", r.NJ), kv("NQ", r.NQ), kv("seg_blocks", r.seg_blocks);
  kv("nsplit", r.nsplit);
}

static MsmShape shape_of(size_t n, int c, int min_chunk, int fixed, int rows, int host, int split, int cache_kb,
                         int chunk_kb) {
  MsmShape sh{};
  sh.n = n;
  sh.fixed = fixed != 0;
  sh.npad = fixed ? std::max<size_t>(kSortB, sort_round(n)) : 0;  // fixed_table_impl's npad
  sh.fixed_c = fixed ? c : 0;
  sh.rows = fixed ? rows : 1;
  sh.host_scalars = host != 0;
  sh.window_c = c;
  sh.min_chunk = min_chunk;
  sh.split_copy = split;
  sh.fine_cache_kb = cache_kb;
  sh.fine_chunk_kb = chunk_kb;
  return sh;
}

static void dump_schedule(const MsmSchedule& s) {
  kv("err", s.err), kv("kmerge", s.kmerge), kv("d16", s.d16), kv("nch", s.parts.nch);
  dump_plan(s.pl);
  dump_reduce(s.red);
  for (int ch = 0; ch < s.parts.nch; ch++) {
    const SortPlan& q = s.part[ch];
    const std::string p = "p" + std::to_string(ch) + "_";
    kvs(p + "err", q.err), kvs(p + "c0", q.c0), kvs(p + "nc", q.nc), kvs(p + "stride", q.stride);
    kvs(p + "E", q.E), kvs(p + "nW", q.nW), kvs(p + "TOTB", q.TOTB);
    dump_geom(p + "g_", q.g);
    dump_geom(p + "gm_", q.gm);
    kvs(p + "tiles_chunk", q.tiles.chunk), kvs(p + "tiles_R", q.tiles.R), kvs(p + "tiles_nblk", q.tiles.nblk);
    kvs(p + "tiles_rows", q.tiles.rows), kvs(p + "nb", q.nb), kvs(p + "wide", q.wide);
    kvs(p + "lds_coarse", q.lds_coarse), kvs(p + "cache_n", q.cache_n), kvs(p + "chn", q.chn);
    kvs(p + "lds_fine", q.lds_fine), kvs(p + "chunk", q.chunk), kvs(p + "nthreads", q.nthreads);
  }
}

static void pairing_query() {
  namespace pp = pm::pairing;
  kv("kSteps", pp::kSteps), kv("kProgOps", pp::kProgOps), kv("n", pp::kProgram.n), kv("kSlots", pp::kSlots);
  kv("kPairG", pp::kPairG), kv("kPairPerBlock", pp::kPairPerBlock), kv("kLdsWords", pp::kLdsWords);
  kv("kOpMul", pp::kOpMul), kv("kOpLine", pp::kOpLine), kv("kOpFrob", pp::kOpFrob), kv("kOpConj", pp::kOpConj);
  kv("kOpScaleInv", pp::kOpScaleInv);
  list("prog", std::vector<uint32_t>(pp::kProgram.w, pp::kProgram.w + pp::kProgOps));
  std::vector<uint32_t> dbl;
  for (int s = 0; s < pp::kSteps; s++) dbl.push_back(pp::step_doubles(s) ? 1u : 0u);
  list("doubles", dbl);
  std::printf("frob=");
  const uint64_t* f = &pp::kFrob[0][0][0][0];
  for (int i = 0; i < 2 * 6 * 2 * 4; i++) std::printf(i ? ",%llu" : "%llu", (unsigned long long)f[i]);
  std::printf(" ");
}

static bool terms_query(std::istringstream& in) {
  uint32_t nfixed, nperm, qdeg, p_h, p_W, nsets;
  if (!(in >> nfixed >> nperm >> qdeg >> p_h >> p_W >> nsets)) return false;
  pm_proof_shape s{};
  s.num_fixed_columns = nfixed;
  s.n_perm_columns = nperm;
  s.quotient_degree = qdeg;
  AccLayout L{};
  L.p_h = p_h;
  L.p_W = p_W;
  L.nsets = nsets;
  std::vector<std::vector<AccQuery>> sets(nsets);
  for (auto& st : sets) {
    uint32_t len;
    if (!(in >> len)) return false;
    st.resize(len);
    for (auto& q : st) {
      if (!(in >> q.ref_kind >> q.ref_idx >> q.eval)) return false;
      q.rot = 0;
    }
  }
  AccTerms t;
  acc_terms(&s, L, sets, t);
  kv("T", t.T), kv("Tp", t.Tp), kv("nslots", t.nslots), kv("h_slot0", t.h_slot0), kv("npair", t.npair);
  list("termsrc", t.termsrc), list("qprog", t.qprog), list("pairs", t.pairs);
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    std::vector<long long> a;
    bool ok = true;
    if (cmd == "terms") {
      ok = terms_query(in);
    } else {
      for (long long v; in >> v;) a.push_back(v);
      const size_t na = a.size();
      if (cmd == "consts" && na == 0) {
        consts();
      } else if (cmd == "pairing" && na == 0) {
        pairing_query();
      } else if (cmd == "msm" && na == 3) {
        dump_plan(make_plan((size_t)a[0], (int)a[1], (int)a[2]));
      } else if (cmd == "parts" && na == 4) {
        const MsmParts p = msm_parts((size_t)a[0], a[1] != 0, a[2] != 0, (int)a[3]);
        kv("nch", p.nch);
        list("pstart", std::vector<uint32_t>(p.pstart, p.pstart + p.nch + 1));
      } else if (cmd == "sort" && na == 9) {
        dump_schedule(msm_schedule(shape_of((size_t)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5],
                                            (int)a[6], (int)a[7], (int)a[8])));
      } else if (cmd == "reduce" && na == 5) {
        const MsmShape sh = shape_of((size_t)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], 0, 0, 0, 0);
        const MsmPlan pl = sh.fixed ? make_plan_fixed(sh.npad, sh.fixed_c, sh.min_chunk)
                                    : make_plan(sh.n, sh.window_c, sh.min_chunk);
        dump_reduce(reduce_plan(pl, sh.rows));
      } else if (cmd == "small" && na == 1) {
        const SmallPlan p = small_plan((size_t)a[0]);
        std::printf("path=%s ", p.fused ? "fused" : p.lanes ? "lanes" : "quads");
        kv("fused", p.fused), kv("lanes", p.lanes), kv("kq", p.kq), kv("ns", p.ns);
      } else if (cmd == "many" && na == 1) {
        const uint32_t c = many_pick_c((size_t)a[0]);
        kv("c", c), kv("W", many_windows(c)), kv("bytes_per_base", many_bytes_per_base(c));
      } else if (cmd == "manyc" && na == 1) {
        kv("W", many_windows((uint32_t)a[0])), kv("bytes_per_base", many_bytes_per_base((uint32_t)a[0]));
      } else if (cmd == "manykq" && na == 1) {
        kv("kq", many_kq((size_t)a[0]));
      } else if (cmd == "acc" && (na == 7 || na == 11)) {
        AccPathIn in2;
        in2.B = (size_t)a[0], in2.T = (uint32_t)a[1], in2.Tp = (uint32_t)a[2], in2.npair = (uint32_t)a[3];
        in2.split = (int)a[4], in2.tpl = (int)a[5], in2.ladder = (int)a[6];
        if (na == 11)
          in2.nvk_build = (size_t)a[7], in2.row_bytes = (size_t)a[8], in2.tail_bytes = (size_t)a[9],
          in2.lds_cap = (size_t)a[10];
        const AccPath p = acc_path(in2);
        kv("lgS", p.lgS), kv("quad_terms", p.quad_terms), kv("lgT", p.lgT), kv("tpl", (unsigned)p.tpl);
        kv("pstep", p.pstep), kv("lgL", p.lgL), kv("sliced", p.sliced), kv("np", p.np), kv("lds", p.lds);
      } else {
        ok = false;
      }
    }
    if (!ok) {
      std::printf("error=bad query: %s\n", line.c_str());
      return 2;
    }
    std::printf("\n");
  }
  return 0;
}
