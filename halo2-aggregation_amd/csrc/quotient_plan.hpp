// quotient_plan.hpp -- host-side compiler of the quotient numerator
// (pm_quotient_*): a pm_proof_shape becomes one linear program
// over a small op set, which k_quot_eval (quotient_kernels.hpp) runs once per
// extended row and quot_eval_host (quotient_engine.hpp) once per point.
//
// The expression list is the one oracle/accum.py::scalar_block builds
// (verifier.rs:593-643, permutation.rs:190-324, lookup.rs:173-311): the
// gates, the permutation identities, five identities per lookup, folded as
// h = h y + e.  The permutation and lookup identities are emitted through the
// same helpers as the gates' postfix code, so the kernel knows one op set.
//
// Machine: value slots (LDS on the device), one fold register h, and three
// read-only tables: leaves, constants, the program.  One u32 per op:
//   op | dst << 4 | a << 10 | b << 16
//   kQLoad   dst = leaf b                      kQConst  dst = constant b
//   kQNeg    dst = -a
//   kQAdd    dst = a + b      (| kQConstB: a + constant b)
//   kQSub    dst = a - b      (| kQConstB: constant b - a)
//   kQMul    dst = a b        (| kQConstB: a x constant b)
//   kQFold   h = h y + a      (b = 1: the first expression, h = a when the
//                              call does not accumulate)
//
// Forms.  f29_mul_c(u, v) = u v 2^-261, and a column holds x 2^256, so a
// product of two columns would be x y 2^251.  Every value carries a deficit d
// known at compile time: its words hold x 2^(261 - 5 d).  A column has d = 1,
// the quotient's own l_0 / l_last / l_sum columns d = 0, a product d_a + d_b.
// A constant is free to take any form: entry (source, k) of the constant table
// holds v 2^(261 + 5 k), so a product with a constant also repairs a deficit,
// and a sum brings the deeper operand down with one product by 2^(261 + 5 k)
// (kQcOne).  A chain of m column factors therefore costs m - 1 products and
// one repair, as in gp_kernels.hpp.  Every expression reaches the fold at
// d = 1, y is stored at d = 0, and h stays in the columns' form.
//
// Leaves.  The device program keys a leaf by (pointer slot, rot 2^e mod N),
// the host program by the index of the evaluation in pm_shape_layout's scalar
// order (two queries of one cell are two evaluations there).  A leaf that is
// used more than once is loaded once and keeps its slot until its last use,
// unless that needs more than kQuotCacheSlots slots; then every use loads.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "accum_plan.hpp"

namespace pm {

constexpr uint32_t kQuotMaxSlots = 28;     // 28 x 36 B x 64 lanes = 63 KiB of LDS per wave
constexpr uint32_t kQuotCacheSlots = 8;    // leaves stay resident only while the program fits this many
constexpr uint32_t kQuotMaxOps = 1u << 16; // ops; also bounds leaves and constants (16-bit operand)
constexpr uint32_t kQuotMaxLogN = 28;

enum : uint32_t { kQLoad = 0, kQConst = 1, kQNeg = 2, kQAdd = 3, kQSub = 4, kQMul = 5, kQFold = 6, kQConstB = 8 };
// leaf kinds: the pointer groups of a call, in pm_quotient_columns order, then the quotient's own columns
enum : uint32_t {
  kQlAdvice = 0, kQlFixed, kQlInstance, kQlSigma, kQlPermZ, kQlLookupA, kQlLookupS, kQlLookupZ, kQlOwn, kQlKinds
};
enum : uint32_t { kQownL0 = 0, kQownLast = 1, kQownSum = 2, kQownX = 3, kQownCols = 4 };
// constant sources
enum : uint32_t { kQcShape = 0, kQcTheta, kQcBeta, kQcGamma, kQcY, kQcBetaDelta, kQcOne, kQcZero };

struct QuotLeaf {
  uint32_t kind, index;  // pointer group and column in it (kQlOwn: kQown*)
  int32_t rot;
  uint32_t eval;         // host: index into the proof's scalars (kQlOwn: kQown*)
};
struct QuotConst {
  uint32_t src, index;   // kQcShape: constants[index]; kQcBetaDelta: beta delta^index
  int32_t k;             // the entry holds v 2^(261 + 5 k)
  uint32_t neg;          // ... of -v
};
struct QuotPlan {
  std::vector<uint32_t> ops;
  std::vector<QuotLeaf> leaves;
  std::vector<QuotConst> consts;
  uint32_t group_base[kQlKinds + 1] = {};  // first pointer slot of each group
  uint32_t slots = 0, n_expr = 0, products = 0, loads = 0, y_const = 0;
  bool cached = false;                     // repeated leaves keep their slot
  bool need_l = false, need_x = false;     // the program reads l_0 / l_last / l_sum, X
};

struct QuotVal {
  int slot;  // < 0: a constant that is in no slot yet
  int d;
  uint32_t csrc, cidx;
};

class QuotCompiler {
 public:
  // ext_shift < 0: host keys (one leaf per evaluation); else e = extended_k - k of the device program
  QuotCompiler(const pm_proof_shape* s, const AccLayout& L, int ext_shift, uint32_t log_ext)
      : s_(s), L_(L), e_(ext_shift), logN_(log_ext) {}

  // "" on success; *unsupported tells PM_ERR_UNSUPPORTED from PM_ERR_ARG
  std::string compile(QuotPlan* out, uint32_t cache_slots, bool* unsupported) {
    *unsupported = false;
    std::vector<uint32_t> no_uses;
    QuotPlan plain;
    std::string err = pass(&plain, false, no_uses);
    if (!err.empty()) return err;
    *out = plain;
    if (cache_slots) {
      const std::vector<uint32_t> uses = uses_;
      QuotPlan cached;
      err = pass(&cached, true, uses);
      if (err.empty() && cached.slots <= cache_slots && cached.ops.size() <= kQuotMaxOps) *out = cached;
    }
    if (out->n_expr == 0) return "no expressions";
    *unsupported = true;
    if (out->ops.size() > kQuotMaxOps) return "program longer than 65536 ops";
    if (out->leaves.size() > kQuotMaxOps || out->consts.size() > kQuotMaxOps) return "more than 65536 leaves or constants";
    if (out->slots > kQuotMaxSlots) return "program needs more than 28 value slots";
    *unsupported = false;
    return "";
  }

 private:
  const pm_proof_shape* s_;
  AccLayout L_;
  int e_;
  uint32_t logN_;
  QuotPlan* p_ = nullptr;
  bool cache_ = false;
  std::vector<uint32_t> uses_;       // per leaf: uses counted by this pass
  std::vector<uint32_t> left_;       // cached pass: uses not yet emitted
  std::vector<int> leaf_slot_;       // cached pass: the slot a leaf sits in, or -1
  std::vector<uint32_t> refs_;       // per slot
  std::vector<int> slot_leaf_;       // per slot: the leaf it caches, or -1
  std::map<std::pair<uint64_t, uint64_t>, uint32_t> leaf_ids_;
  std::map<std::vector<int64_t>, uint32_t> const_ids_;
  bool first_fold_ = true;
  std::string err_;

  void emit(uint32_t op, uint32_t dst, uint32_t a, uint32_t b) {
    if (b >= kQuotMaxOps && err_.empty()) err_ = "operand index above 65535";
    p_->ops.push_back(op | dst << 4 | a << 10 | b << 16);
    if ((op & 7u) == kQMul) p_->products++;
  }
  int alloc() {
    for (size_t i = 0; i < refs_.size(); i++)
      if (!refs_[i]) {
        refs_[i] = 1;
        return (int)i;
      }
    refs_.push_back(1);
    slot_leaf_.push_back(-1);
    if (refs_.size() > 63 && err_.empty()) err_ = "more than 63 value slots";
    p_->slots = std::max<uint32_t>(p_->slots, (uint32_t)refs_.size());
    return (int)refs_.size() - 1;
  }
  void forget_leaf(int slot) {
    if (slot_leaf_[slot] >= 0) {
      leaf_slot_[slot_leaf_[slot]] = -1;
      slot_leaf_[slot] = -1;
    }
  }
  void release(const QuotVal& v) {
    if (v.slot < 0) return;
    if (--refs_[v.slot] == 0) forget_leaf(v.slot);
  }
  // destination of an op that consumes a (and b): an operand's slot when this is its last use
  int take_dst(const QuotVal& a, const QuotVal* b) {
    if (a.slot >= 0 && refs_[a.slot] == 1) {
      forget_leaf(a.slot);
      if (b) release(*b);
      return a.slot;
    }
    if (b && b->slot >= 0 && refs_[b->slot] == 1) {
      forget_leaf(b->slot);
      release(a);
      return b->slot;
    }
    const int dst = alloc();
    release(a);
    if (b) release(*b);
    return dst;
  }
  uint32_t cid(uint32_t src, uint32_t idx, int k, bool neg) {
    const std::vector<int64_t> key = {(int64_t)src, (int64_t)idx, (int64_t)k, neg ? 1 : 0};
    auto it = const_ids_.find(key);
    if (it != const_ids_.end()) return it->second;
    const uint32_t id = (uint32_t)p_->consts.size();
    p_->consts.push_back({src, idx, k, neg ? 1u : 0u});
    const_ids_[key] = id;
    return id;
  }
  static QuotVal konst(uint32_t src, uint32_t idx = 0) { return {-1, 1, src, idx}; }

  QuotVal leaf(uint32_t kind, uint32_t index, int32_t rot, uint32_t eval) {
    std::pair<uint64_t, uint64_t> key;
    if (e_ < 0) {
      key = {kind == kQlOwn ? 1u : 0u, eval};
    } else {
      const uint64_t mask = ((uint64_t)1 << logN_) - 1;
      key = {p_->group_base[kind] + index, (uint64_t)((int64_t)rot * ((int64_t)1 << e_)) & mask};
    }
    uint32_t id;
    auto it = leaf_ids_.find(key);
    if (it == leaf_ids_.end()) {
      id = (uint32_t)p_->leaves.size();
      p_->leaves.push_back({kind, index, rot, eval});
      leaf_ids_[key] = id;
      uses_.push_back(0);
      leaf_slot_.push_back(-1);
    } else {
      id = it->second;
    }
    uses_[id]++;
    if (kind == kQlOwn) (index == kQownX ? p_->need_x : p_->need_l) = true;
    const int d = kind == kQlOwn && index != kQownX ? 0 : 1;
    if (cache_ && leaf_slot_[id] >= 0) {
      left_[id]--;
      return {leaf_slot_[id], d, 0, 0};
    }
    const int slot = alloc();
    emit(kQLoad, (uint32_t)slot, 0, id);
    p_->loads++;
    if (cache_ && left_[id] > 1) {
      refs_[slot] = left_[id];
      leaf_slot_[id] = slot;
      slot_leaf_[slot] = (int)id;
    }
    if (cache_) left_[id]--;
    return {slot, d, 0, 0};
  }

  QuotVal in_slot(QuotVal v, int d) {
    if (v.slot >= 0) return v;
    const int slot = alloc();
    emit(kQConst, (uint32_t)slot, 0, cid(v.csrc, v.cidx, -d, false));
    return {slot, d, 0, 0};
  }
  // bring a slot value to deficit d: one product by 2^(261 + 5 (v.d - d))
  QuotVal fix(QuotVal v, int d) {
    if (v.slot < 0 || v.d == d) return v;
    const uint32_t c = cid(kQcOne, 0, v.d - d, false);
    const int dst = take_dst(v, nullptr);
    emit(kQMul | kQConstB, (uint32_t)dst, (uint32_t)v.slot, c);
    return {dst, d, 0, 0};
  }
  QuotVal neg(QuotVal v) {
    v = in_slot(v, 1);
    const int dst = take_dst(v, nullptr);
    emit(kQNeg, (uint32_t)dst, (uint32_t)v.slot, 0);
    return {dst, v.d, 0, 0};
  }
  // a + b, or a - b (minus)
  QuotVal add(QuotVal a, QuotVal b, bool minus = false) {
    if (a.slot < 0 && b.slot < 0) a = in_slot(a, 1);
    if (b.slot < 0) {  // a +- constant
      const int dst = take_dst(a, nullptr);
      emit(kQAdd | kQConstB, (uint32_t)dst, (uint32_t)a.slot, cid(b.csrc, b.cidx, -a.d, minus));
      return {dst, a.d, 0, 0};
    }
    if (a.slot < 0) {  // constant +- b
      const int dst = take_dst(b, nullptr);
      emit((minus ? kQSub : kQAdd) | kQConstB, (uint32_t)dst, (uint32_t)b.slot, cid(a.csrc, a.cidx, -b.d, false));
      return {dst, b.d, 0, 0};
    }
    const int d = std::min(a.d, b.d);
    if (a.d != d) a = fix(a, d);
    if (b.d != d) b = fix(b, d);
    const uint32_t sa = (uint32_t)a.slot, sb = (uint32_t)b.slot;
    const int dst = take_dst(a, &b);
    emit(minus ? kQSub : kQAdd, (uint32_t)dst, sa, sb);
    return {dst, d, 0, 0};
  }
  QuotVal sub(QuotVal a, QuotVal b) { return add(a, b, true); }
  QuotVal mul(QuotVal a, QuotVal b) {
    if (a.slot < 0 && b.slot < 0) a = in_slot(a, 1);
    if (a.slot < 0) std::swap(a, b);
    if (b.slot < 0) {  // the constant's form absorbs a deficit above 1
      const int d = std::min(a.d, 1);
      const uint32_t c = cid(b.csrc, b.cidx, a.d - d, false);
      const uint32_t sa = (uint32_t)a.slot;
      const int dst = take_dst(a, nullptr);
      emit(kQMul | kQConstB, (uint32_t)dst, sa, c);
      return {dst, d, 0, 0};
    }
    const uint32_t sa = (uint32_t)a.slot, sb = (uint32_t)b.slot;
    const int d = a.d + b.d;
    const int dst = take_dst(a, &b);
    emit(kQMul, (uint32_t)dst, sa, sb);
    return {dst, d, 0, 0};
  }
  void fold(QuotVal e) {
    e = in_slot(fix(e, 1), 1);
    emit(kQFold, 0, (uint32_t)e.slot, first_fold_ ? 1u : 0u);
    if (!first_fold_) p_->products++;
    first_fold_ = false;
    release(e);
    p_->n_expr++;
  }

  QuotVal query_leaf(uint32_t op, uint32_t q) {
    if (op == PM_EXPR_FIXED) return leaf(kQlFixed, s_->fixed_queries[q].column, s_->fixed_queries[q].rotation, L_.s_fixed + q);
    if (op == PM_EXPR_ADVICE)
      return leaf(kQlAdvice, s_->advice_queries[q].column, s_->advice_queries[q].rotation, L_.s_adv + q);
    return leaf(kQlInstance, s_->instance_queries[q].column, s_->instance_queries[q].rotation, L_.s_inst + q);
  }
  // the validated postfix code, one call of `done` per expression
  template <class F>
  void run_code(const uint32_t* code, uint32_t len, F done) {
    std::vector<QuotVal> st;
    for (uint32_t i = 0; i < len; i++) {
      const uint32_t op = code[i] & 0xffu, arg = code[i] >> 8;
      switch (op) {
        case PM_EXPR_CONST: st.push_back(konst(kQcShape, arg)); break;
        case PM_EXPR_FIXED:
        case PM_EXPR_ADVICE:
        case PM_EXPR_INSTANCE: st.push_back(query_leaf(op, arg)); break;
        case PM_EXPR_NEG: st.back() = neg(st.back()); break;
        case PM_EXPR_SUM:
        case PM_EXPR_PROD: {
          const QuotVal b = st.back();
          st.pop_back();
          st.back() = op == PM_EXPR_SUM ? add(st.back(), b) : mul(st.back(), b);
          break;
        }
        case PM_EXPR_SCALED: st.back() = mul(st.back(), konst(kQcShape, arg)); break;
        default:  // PM_EXPR_END
          done(st.back());
          st.pop_back();
      }
    }
  }
  // lookup.rs compress_expressions: Horner in theta from zero over the flattened list
  QuotVal compress(const uint32_t* code, uint32_t len) {
    bool any = false;
    QuotVal acc = konst(kQcZero);
    run_code(code, len, [&](QuotVal v) {
      acc = any ? add(mul(acc, konst(kQcTheta)), v) : v;
      any = true;
    });
    return acc;
  }
  QuotVal perm_value(uint32_t k) {
    const pm_perm_column& c = s_->perm_columns[k];
    return query_leaf(c.kind == PM_COL_ADVICE ? PM_EXPR_ADVICE : c.kind == PM_COL_FIXED ? PM_EXPR_FIXED : PM_EXPR_INSTANCE,
                      c.query_index);
  }
  QuotVal own(uint32_t which) { return leaf(kQlOwn, which, 0, which); }
  // 1 - (l_last + l_blind), d = 0
  QuotVal active() { return sub(konst(kQcOne), own(kQownSum)); }
  // z^2 - z as z (z - 1)
  QuotVal boolean(uint32_t kind, uint32_t idx, uint32_t eval) {
    return mul(sub(leaf(kind, idx, 0, eval), konst(kQcOne)), leaf(kind, idx, 0, eval));
  }

  void permutation() {
    const uint32_t nps = L_.n_perm_sets, cl = s_->perm_chunk_len;
    if (!nps) return;
    const int32_t last_rot = -(int32_t)(s_->blinding_factors + 1);
    auto z = [&](uint32_t i, int32_t rot, uint32_t which) { return leaf(kQlPermZ, i, rot, L_.s_perm + 3 * i + which); };
    fold(mul(sub(konst(kQcOne), z(0, 0, 0)), own(kQownL0)));
    fold(mul(boolean(kQlPermZ, nps - 1, L_.s_perm + 3 * (nps - 1)), own(kQownLast)));
    for (uint32_t i = 1; i < nps; i++) fold(mul(sub(z(i, 0, 0), z(i - 1, last_rot, 2)), own(kQownL0)));
    for (uint32_t ci = 0; ci < nps; ci++) {
      const uint32_t k0 = ci * cl, k1 = std::min(s_->n_perm_columns, k0 + cl);
      QuotVal left = z(ci, 1, 1);
      for (uint32_t k = k0; k < k1; k++) {
        const QuotVal sig = mul(leaf(kQlSigma, k, 0, L_.s_sigma + k), konst(kQcBeta));
        left = mul(left, add(add(sig, perm_value(k)), konst(kQcGamma)));
      }
      QuotVal right = z(ci, 0, 0);
      for (uint32_t k = k0; k < k1; k++) {
        const QuotVal t = mul(own(kQownX), konst(kQcBetaDelta, k));
        right = mul(right, add(add(t, perm_value(k)), konst(kQcGamma)));
      }
      fold(mul(sub(left, right), active()));
    }
  }

  void lookup(uint32_t i) {
    const uint32_t ev = L_.s_lk + 5 * i;
    auto z = [&] { return leaf(kQlLookupZ, i, 0, ev + 0); };
    auto a = [&] { return leaf(kQlLookupA, i, 0, ev + 2); };
    auto sp = [&] { return leaf(kQlLookupS, i, 0, ev + 4); };
    fold(mul(sub(konst(kQcOne), z()), own(kQownL0)));
    fold(mul(boolean(kQlLookupZ, i, ev + 0), own(kQownLast)));
    QuotVal left = mul(add(a(), konst(kQcBeta)), add(sp(), konst(kQcGamma)));
    left = mul(left, leaf(kQlLookupZ, i, 1, ev + 1));
    const QuotVal cin = add(compress(s_->lookup_input_code, s_->lookup_input_code_len), konst(kQcBeta));
    const QuotVal ctab = add(compress(s_->lookup_table_code, s_->lookup_table_code_len), konst(kQcGamma));
    const QuotVal right = mul(mul(cin, ctab), z());
    fold(mul(sub(left, right), active()));
    fold(mul(sub(a(), sp()), own(kQownL0)));
    const QuotVal step = sub(a(), leaf(kQlLookupA, i, -1, ev + 3));
    fold(mul(mul(sub(a(), sp()), step), active()));
  }

  std::string pass(QuotPlan* out, bool cache, const std::vector<uint32_t>& uses) {
    p_ = out;
    cache_ = cache;
    left_ = uses;
    uses_.clear();
    leaf_slot_.clear();
    refs_.clear();
    slot_leaf_.clear();
    leaf_ids_.clear();
    const_ids_.clear();
    first_fold_ = true;
    err_.clear();
    out->cached = cache;
    const uint32_t counts[kQlKinds] = {s_->num_advice_columns, s_->num_fixed_columns, s_->num_instance_columns,
                                       s_->n_perm_columns,     L_.n_perm_sets,        s_->num_lookups,
                                       s_->num_lookups,        s_->num_lookups,       kQownCols};
    for (uint32_t g = 0; g < kQlKinds; g++) out->group_base[g + 1] = out->group_base[g] + counts[g];
    run_code(s_->gate_code, s_->gate_code_len, [&](QuotVal v) { fold(v); });
    permutation();
    for (uint32_t i = 0; i < s_->num_lookups; i++) lookup(i);
    out->y_const = cid(kQcY, 0, 0, false);
    return err_;
  }
};

// Validates the shape and compiles it; ext_shift < 0 selects the host keys.
inline std::string quot_compile(const pm_proof_shape* s, int ext_shift, uint32_t log_ext, uint32_t cache_slots,
                                QuotPlan* plan, AccLayout* layout, bool* unsupported) {
  std::vector<AccQuery> q;
  *unsupported = false;
  const std::string err = acc_validate(s, q, *layout, nullptr);
  if (!err.empty()) return err;
  QuotCompiler c(s, *layout, ext_shift, log_ext);
  return c.compile(plan, cache_slots, unsupported);
}

}  // namespace pm
