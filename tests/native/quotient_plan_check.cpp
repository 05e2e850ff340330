// Host check of csrc/quotient_plan.hpp (built by tests/test_quotient_plan.py
// with g++ and the address / undefined-behaviour sanitizers): compiles a few
// shapes with host keys and with device keys at e = 0 .. 3, with repeated
// leaves reloaded (0), resident under the default bound (8) and resident up
// to the slot budget (28), and walks every program with an abstract
// interpreter that knows nothing of the compiler's bookkeeping:
//   * every slot, leaf and constant index is in range, no slot is read before
//     it is written, the first fold and only the first carries the flag;
//   * the forms are consistent: with d(column) = 1, d(l columns) = 0,
//     d(constant entry k) = -k, a sum takes equal deficits, a product adds
//     them, and every expression reaches the fold at d = 1;
//   * the counters pm_quotient_info reports equal the ops counted here.
// Prints one line per shape and "ok"; exits nonzero on the first violation.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../halo2-aggregation_amd/csrc/quotient_plan.hpp"

using namespace pm;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s line %d: %s\n", name, __LINE__, #c);    \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

struct Shape {
  std::vector<pm_query> iq, aq, fq;
  std::vector<pm_perm_column> pc;
  std::vector<uint32_t> gates, lin, ltab;
  std::vector<uint64_t> consts, points;
  pm_proof_shape s{};
  const pm_proof_shape* finish(uint32_t ni, uint32_t na, uint32_t nf, uint32_t nl, uint32_t chunk, uint32_t bf) {
    points.assign(8 * (nf + pc.size() + 1), 0);
    s.log_n = 6;
    s.blinding_factors = bf;
    s.num_instance_columns = ni;
    s.num_advice_columns = na;
    s.num_fixed_columns = nf;
    s.num_lookups = nl;
    s.perm_chunk_len = chunk;
    s.quotient_degree = 2;
    s.n_instance_queries = (uint32_t)iq.size();
    s.n_advice_queries = (uint32_t)aq.size();
    s.n_fixed_queries = (uint32_t)fq.size();
    s.n_perm_columns = (uint32_t)pc.size();
    s.instance_queries = iq.data();
    s.advice_queries = aq.data();
    s.fixed_queries = fq.data();
    s.perm_columns = pc.data();
    s.gate_code = gates.data();
    s.gate_code_len = (uint32_t)gates.size();
    s.lookup_input_code = lin.data();
    s.lookup_input_code_len = (uint32_t)lin.size();
    s.lookup_table_code = ltab.data();
    s.lookup_table_code_len = (uint32_t)ltab.size();
    s.constants = consts.data();
    s.n_constants = (uint32_t)(consts.size() / 4);
    s.fixed_commitments = points.data();
    s.sigma_commitments = points.data();
    return &s;
  }
};

static uint32_t op(uint32_t o, uint32_t arg = 0) { return o | arg << 8; }

static void walk(const char* name, const pm_proof_shape* s, const QuotPlan& p) {
  std::vector<int> d(p.slots, 0);
  std::vector<bool> set(p.slots, false);
  uint32_t folds = 0, loads = 0, products = 0;
  for (uint32_t w : p.ops) {
    const uint32_t o = w & 7u, cb = w & kQConstB, dst = (w >> 4) & 63u, a = (w >> 10) & 63u, b = w >> 16;
    if (o == kQLoad) {
      CHECK(dst < p.slots && b < p.leaves.size());
      const QuotLeaf& lf = p.leaves[b];
      CHECK(lf.kind < kQlKinds && p.group_base[lf.kind] + lf.index < p.group_base[lf.kind + 1]);
      d[dst] = lf.kind == kQlOwn && lf.index != kQownX ? 0 : 1;
      set[dst] = true;
      loads++;
      continue;
    }
    if (o == kQConst) {
      CHECK(dst < p.slots && b < p.consts.size());
      d[dst] = -p.consts[b].k;
      set[dst] = true;
      continue;
    }
    CHECK(a < p.slots && set[a]);
    if (o == kQFold) {
      CHECK(d[a] == 1 && b == (folds == 0 ? 1u : 0u));
      folds++;
      continue;
    }
    CHECK(dst < p.slots);
    int db = 0;
    if (o != kQNeg) {
      if (cb) {
        CHECK(b < p.consts.size());
        db = -p.consts[b].k;
        if (p.consts[b].src == kQcShape) CHECK(p.consts[b].index < s->n_constants);
      } else {
        CHECK(b < p.slots && set[b]);
        db = d[b];
      }
    }
    if (o == kQMul) {
      d[dst] = d[a] + db;
      products++;
    } else if (o == kQAdd || o == kQSub) {
      CHECK(d[a] == db);
      d[dst] = d[a];
    } else {
      CHECK(o == kQNeg);
      d[dst] = d[a];
    }
    set[dst] = true;
  }
  CHECK(folds == p.n_expr && loads == p.loads && products + folds - 1 == p.products);
  CHECK(p.y_const < p.consts.size() && p.consts[p.y_const].src == kQcY && p.consts[p.y_const].k == 0);
}

static void run(const char* name, const pm_proof_shape* s, uint32_t want_expr) {
  uint32_t reload_loads = 0;
  for (int e = -1; e <= 3; e++) {
    for (uint32_t cache : {0u, kQuotCacheSlots, kQuotMaxSlots}) {
      QuotPlan p;
      AccLayout L;
      bool unsupported = false;
      const std::string err = quot_compile(s, e, s->log_n + (e < 0 ? 0 : e), cache, &p, &L, &unsupported);
      if (!err.empty()) std::printf("FAIL %s: %s\n", name, err.c_str());
      CHECK(err.empty() && !unsupported);
      CHECK(p.n_expr == want_expr && p.slots >= 1 && p.slots <= kQuotMaxSlots);
      CHECK(cache || !p.cached);
      CHECK(!p.cached || p.slots <= cache);
      walk(name, s, p);
      if (e == -1 && cache == 0) reload_loads = p.loads;
      if (e == -1) CHECK(p.loads <= reload_loads);
      if (e == -1 && cache == kQuotMaxSlots)
        std::printf("%s: %zu ops, %u products, loads %u -> %u, slots %u\n", name, p.ops.size(), p.products,
                    reload_loads, p.loads, p.slots);
    }
  }
}

int main() {
  {  // the simple-example shape
    Shape x;
    x.iq = {{0, 0}};
    x.aq = {{0, 0}, {1, 0}, {0, 1}};
    x.fq = {{0, 0}, {1, 0}, {2, 0}, {3, 0}};
    x.pc = {{PM_COL_INSTANCE, 0}, {PM_COL_FIXED, 0}, {PM_COL_ADVICE, 0}, {PM_COL_ADVICE, 1}};
    x.gates = {op(PM_EXPR_FIXED, 2), op(PM_EXPR_ADVICE, 0), op(PM_EXPR_ADVICE, 1), op(PM_EXPR_PROD),
               op(PM_EXPR_ADVICE, 2), op(PM_EXPR_NEG), op(PM_EXPR_SUM), op(PM_EXPR_PROD), op(PM_EXPR_END)};
    x.lin = {op(PM_EXPR_FIXED, 3), op(PM_EXPR_ADVICE, 0), op(PM_EXPR_PROD), op(PM_EXPR_END)};
    x.ltab = {op(PM_EXPR_FIXED, 1), op(PM_EXPR_END)};
    run("simple", x.finish(1, 2, 4, 1, 3, 5), 1 + 5 + 5);
  }
  {  // three permutation sets, two lookups over two expressions each, constants, negative rotations
    Shape x;
    x.iq = {{0, 0}, {1, -2}};
    x.aq = {{0, 0}, {1, 0}, {2, 0}, {0, 1}, {2, -1}, {0, 0}};
    x.fq = {{0, 0}, {1, 1}};
    for (uint32_t k = 0; k < 7; k++) x.pc.push_back({(uint32_t)(k % 3 == 2 ? PM_COL_FIXED : PM_COL_ADVICE), k % 2});
    x.consts.assign(4 * 3, 7);
    x.gates = {op(PM_EXPR_CONST, 0), op(PM_EXPR_CONST, 1), op(PM_EXPR_PROD), op(PM_EXPR_END),
               op(PM_EXPR_ADVICE, 5), op(PM_EXPR_ADVICE, 0), op(PM_EXPR_PROD), op(PM_EXPR_SCALED, 2), op(PM_EXPR_NEG),
               op(PM_EXPR_CONST, 0), op(PM_EXPR_SUM), op(PM_EXPR_END), op(PM_EXPR_CONST, 1), op(PM_EXPR_NEG),
               op(PM_EXPR_END)};
    x.lin = {op(PM_EXPR_ADVICE, 0), op(PM_EXPR_END), op(PM_EXPR_CONST, 2), op(PM_EXPR_END)};
    x.ltab = {op(PM_EXPR_FIXED, 1), op(PM_EXPR_INSTANCE, 1), op(PM_EXPR_SUM), op(PM_EXPR_END), op(PM_EXPR_FIXED, 0),
              op(PM_EXPR_END)};
    run("rich", x.finish(2, 3, 2, 2, 3, 3), 3 + 7 + 10);
  }
  for (int prod = 0; prod < 2; prod++) {  // 16 leaves, right- and left-leaning: postfix stack 16 and 2
    Shape x;
    x.aq = {{0, 0}, {1, 0}, {2, 1}};
    for (int i = 0; i < 16; i++) x.gates.push_back(op(PM_EXPR_ADVICE, i % 3));
    for (int i = 0; i < 15; i++) x.gates.push_back(op(prod ? PM_EXPR_PROD : PM_EXPR_SUM));
    x.gates.push_back(op(PM_EXPR_END));
    x.gates.push_back(op(PM_EXPR_ADVICE, 0));
    for (int i = 1; i < 16; i++) {
      x.gates.push_back(op(PM_EXPR_ADVICE, i % 3));
      x.gates.push_back(op(prod ? PM_EXPR_PROD : PM_EXPR_SUM));
    }
    x.gates.push_back(op(PM_EXPR_END));
    run(prod ? "depth16_products" : "depth16_sums", x.finish(0, 3, 0, 0, 0, 1), 2);
  }
  {  // lookups with empty expression lists: the compress of nothing is zero
    Shape x;
    x.aq = {{0, 0}};
    run("empty_lookup_lists", x.finish(0, 1, 0, 1, 0, 2), 5);
  }
  std::printf("ok\n");
  return 0;
}
