// accum_plan.hpp -- host-side plan of the batch multiopen accumulator.
//
// From a pm_proof_shape (the VerifyingKey / ConstraintSystem view of
// /root/reference/src/verifier.rs:227-285) this builds, once per call, the
// query list in the reference order (verifier.rs:654-715 with
// permutation.rs:332-358, lookup.rs:314-347, vanishing.rs:206-220), groups it
// by rotation like construct_intermediate_sets (src/multiopen.rs:19-45:
// BTreeMap => ascending rotation, query order kept inside a set), and assigns
// every distinct commitment of `f` an MSM term slot.  The device kernels
// (accum_kernels.hpp) only follow this table.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pasta_msm.h"

namespace pm {

// point reference kinds in the query list
enum : uint32_t { kRefProof = 0, kRefFixed = 1, kRefSigma = 2, kRefH = 3 };
constexpr uint32_t kEvalH = 0xFFFFFFFFu;  // query eval = computed h_eval
constexpr uint32_t kSlotH = 0xFFFFu;      // query point = H (vanishing.rs:178-188)
constexpr uint32_t kAccStack = 16;        // expression stack depth bound
constexpr uint32_t kAccMaxSets = 64;
constexpr uint32_t kAccMaxPerSet = 256;
constexpr uint32_t kAccMaxBlind = 61;     // l_i batch of bf + 3 inversions

struct AccQuery {
  uint32_t ref_kind, ref_idx;  // point
  int32_t rot;
  uint32_t eval;               // index into the proof's scalars, or kEvalH
};

// Per-proof layout (transcript read order, see oracle/accum.py)
struct AccLayout {
  uint32_t p_inst, p_adv, p_lkperm, p_permz, p_lkz, p_rand, p_h, p_W, npts;
  uint32_t s_inst, s_adv, s_fixed, s_rand, s_sigma, s_perm, s_lk, nsc;
  uint32_t n_perm_sets, nsets;
};

inline uint32_t acc_perm_sets(const pm_proof_shape* s) {
  return s->perm_chunk_len ? (s->n_perm_columns + s->perm_chunk_len - 1) / s->perm_chunk_len : 0;
}

// Validates the shape and returns the query list + layout; "" on success.
inline std::string acc_build_queries(const pm_proof_shape* s, std::vector<AccQuery>& q, AccLayout& L) {
  if (!s) return "null shape";
  if (s->n_perm_columns && !s->perm_chunk_len) return "perm_chunk_len = 0 with permutation columns";
  if (s->quotient_degree == 0) return "quotient_degree must be >= 1";
  if (s->blinding_factors > kAccMaxBlind) return "blinding_factors too large";
  if (s->log_n == 0 || s->log_n > 32) return "log_n out of range";
  if ((s->n_instance_queries && !s->instance_queries) || (s->n_advice_queries && !s->advice_queries) ||
      (s->n_fixed_queries && !s->fixed_queries) || (s->n_perm_columns && !s->perm_columns))
    return "null query / permutation array";
  if ((s->num_fixed_columns && !s->fixed_commitments) || (s->n_perm_columns && !s->sigma_commitments))
    return "null VK commitments";
  const uint32_t nps = acc_perm_sets(s);
  L.p_inst = 0;
  L.p_adv = L.p_inst + s->num_instance_columns;
  L.p_lkperm = L.p_adv + s->num_advice_columns;
  L.p_permz = L.p_lkperm + 2 * s->num_lookups;
  L.p_lkz = L.p_permz + nps;
  L.p_rand = L.p_lkz + s->num_lookups;
  L.p_h = L.p_rand + 1;
  L.p_W = L.p_h + s->quotient_degree;
  L.s_inst = 0;
  L.s_adv = L.s_inst + s->n_instance_queries;
  L.s_fixed = L.s_adv + s->n_advice_queries;
  L.s_rand = L.s_fixed + s->n_fixed_queries;
  L.s_sigma = L.s_rand + 1;
  L.s_perm = L.s_sigma + s->n_perm_columns;
  L.s_lk = L.s_perm + (nps ? 3 * nps - 1 : 0);
  L.nsc = L.s_lk + 5 * s->num_lookups;
  L.n_perm_sets = nps;

  q.clear();
  for (uint32_t i = 0; i < s->n_instance_queries; i++) {
    if (s->instance_queries[i].column >= s->num_instance_columns) return "instance query column out of range";
    q.push_back({kRefProof, L.p_inst + s->instance_queries[i].column, s->instance_queries[i].rotation, L.s_inst + i});
  }
  for (uint32_t i = 0; i < s->n_advice_queries; i++) {
    if (s->advice_queries[i].column >= s->num_advice_columns) return "advice query column out of range";
    q.push_back({kRefProof, L.p_adv + s->advice_queries[i].column, s->advice_queries[i].rotation, L.s_adv + i});
  }
  // permutation.rs:332-358: (Z, cur), (Z, next) per set; (Z, last) for all but the last set, reversed
  const int32_t last_rot = -(int32_t)(s->blinding_factors + 1);
  for (uint32_t i = 0; i < nps; i++) {
    q.push_back({kRefProof, L.p_permz + i, 0, L.s_perm + 3 * i});
    q.push_back({kRefProof, L.p_permz + i, 1, L.s_perm + 3 * i + 1});
  }
  for (int i = (int)nps - 2; i >= 0; i--) q.push_back({kRefProof, L.p_permz + i, last_rot, L.s_perm + 3 * i + 2});
  // lookup.rs:314-347
  for (uint32_t i = 0; i < s->num_lookups; i++) {
    const uint32_t z = L.p_lkz + i, a = L.p_lkperm + 2 * i, sp = a + 1, e = L.s_lk + 5 * i;
    q.push_back({kRefProof, z, 0, e + 0});
    q.push_back({kRefProof, a, 0, e + 2});
    q.push_back({kRefProof, sp, 0, e + 4});
    q.push_back({kRefProof, a, -1, e + 3});
    q.push_back({kRefProof, z, 1, e + 1});
  }
  for (uint32_t i = 0; i < s->n_fixed_queries; i++) {
    if (s->fixed_queries[i].column >= s->num_fixed_columns) return "fixed query column out of range";
    q.push_back({kRefFixed, s->fixed_queries[i].column, s->fixed_queries[i].rotation, L.s_fixed + i});
  }
  for (uint32_t k = 0; k < s->n_perm_columns; k++) q.push_back({kRefSigma, k, 0, L.s_sigma + k});
  // vanishing.rs:206-220
  q.push_back({kRefH, 0, 0, kEvalH});
  q.push_back({kRefProof, L.p_rand, 0, L.s_rand});

  for (uint32_t k = 0; k < s->n_perm_columns; k++) {
    const pm_perm_column& c = s->perm_columns[k];
    const uint32_t lim = c.kind == PM_COL_ADVICE ? s->n_advice_queries
                         : c.kind == PM_COL_FIXED ? s->n_fixed_queries
                         : c.kind == PM_COL_INSTANCE ? s->n_instance_queries : 0;
    if (c.query_index >= lim) return "permutation column query index out of range";
  }
  std::vector<int32_t> rots;
  for (auto& x : q) rots.push_back(x.rot);
  std::sort(rots.begin(), rots.end());
  rots.erase(std::unique(rots.begin(), rots.end()), rots.end());
  if (rots.size() > kAccMaxSets) return "too many rotation sets";
  L.nsets = (uint32_t)rots.size();
  L.npts = L.p_W + L.nsets;
  return "";
}

// Rotation sets: stable grouping by ascending rotation.
inline void acc_group_sets(const std::vector<AccQuery>& q, std::vector<int32_t>& rots,
                           std::vector<std::vector<AccQuery>>& sets) {
  std::map<int32_t, std::vector<AccQuery>> by;
  for (auto& x : q) by[x.rot].push_back(x);
  rots.clear();
  sets.clear();
  for (auto& kv : by) {
    rots.push_back(kv.first);
    sets.push_back(kv.second);
  }
}

// Checks a postfix expression program; returns the number of expressions
// (END words) or -1 with a message.
inline int acc_check_code(const uint32_t* code, uint32_t len, uint32_t n_const, uint32_t n_adv, uint32_t n_fixed,
                          uint32_t n_inst, std::string& err) {
  if (len && !code) {
    err = "null expression code";
    return -1;
  }
  int sp = 0, nexpr = 0;
  for (uint32_t i = 0; i < len; i++) {
    const uint32_t op = code[i] & 0xffu, arg = code[i] >> 8;
    switch (op) {
      case PM_EXPR_CONST:
        if (arg >= n_const) { err = "CONST index out of range"; return -1; }
        sp++;
        break;
      case PM_EXPR_FIXED:
        if (arg >= n_fixed) { err = "FIXED query index out of range"; return -1; }
        sp++;
        break;
      case PM_EXPR_ADVICE:
        if (arg >= n_adv) { err = "ADVICE query index out of range"; return -1; }
        sp++;
        break;
      case PM_EXPR_INSTANCE:
        if (arg >= n_inst) { err = "INSTANCE query index out of range"; return -1; }
        sp++;
        break;
      case PM_EXPR_NEG:
        if (sp < 1) { err = "NEG on empty stack"; return -1; }
        break;
      case PM_EXPR_SUM:
      case PM_EXPR_PROD:
        if (sp < 2) { err = "binary op on short stack"; return -1; }
        sp--;
        break;
      case PM_EXPR_SCALED:
        if (sp < 1 || arg >= n_const) { err = "bad SCALED"; return -1; }
        break;
      case PM_EXPR_END:
        if (sp != 1) { err = "END with stack depth != 1"; return -1; }
        sp = 0;
        nexpr++;
        break;
      default:
        err = "unknown expression op";
        return -1;
    }
    if (sp > (int)kAccStack) {
      err = "expression stack deeper than 16";
      return -1;
    }
  }
  if (sp != 0) {
    err = "expression code does not end with END";
    return -1;
  }
  return nexpr;
}

// Full validation: queries / layout plus the three expression programs.
inline std::string acc_validate(const pm_proof_shape* s, std::vector<AccQuery>& q, AccLayout& L, int* ngates) {
  std::string err = acc_build_queries(s, q, L);
  if (!err.empty()) return err;
  if (s->n_constants && !s->constants) return "null constants";
  const uint32_t ni = s->n_instance_queries, na = s->n_advice_queries, nf = s->n_fixed_queries;
  const int ng = acc_check_code(s->gate_code, s->gate_code_len, s->n_constants, na, nf, ni, err);
  if (ng < 0) return "gate code: " + err;
  if (acc_check_code(s->lookup_input_code, s->lookup_input_code_len, s->n_constants, na, nf, ni, err) < 0)
    return "lookup input code: " + err;
  if (acc_check_code(s->lookup_table_code, s->lookup_table_code_len, s->n_constants, na, nf, ni, err) < 0)
    return "lookup table code: " + err;
  if (ng + L.n_perm_sets + 5 * s->num_lookups == 0) return "no expressions (vanishing.rs:147 asserts >= 1)";
  if (ngates) *ngates = ng;
  return "";
}

// ------------------------------------------------------------ path choice
// Lanes per item for the latency-bound accumulator kernels: the largest
// power of two 2^lg <= 2^maxlg that keeps items * 2^lg within about two
// waves per SIMD of the 1024 on an MI355X.  Term additions: maxlg = 3 (8
// lanes share a term's ~85 table additions; 16 measured no faster at B = 256,
// the wider butterfly and the second wave per SIMD cost what the shorter loop
// saves).
constexpr size_t kAccLaneBudget = 1024 * 2 * 64;
constexpr size_t kAccSumLanes = 16384;
// row-sliced ladder (k_acc_powers_s) up to this many chains: one wave each,
// four per block and one block per CU (kAccSlicedFence), leaving CUs for the
// side stream's transcript / k_acc_scalars blocks (which a ladder block on
// every CU kept waiting until the ladder ended: B = 16 transcript 0.10 ->
// 0.27 ms with 64-thread ladder blocks, profiles/r05/ladder_ab/r05_lad_scaling.jsonl
// against r05_lad_b_auto.jsonl)
constexpr size_t kAccSlicedChains = 800;
inline uint32_t acc_auto_lanes(size_t items, uint32_t maxlg) {
  uint32_t lg = 0;
  while (lg < maxlg && (items << (lg + 1)) <= kAccLaneBudget) lg++;
  return lg;
}

// The MSM term slots of one proof (accum_device_impl's plan): one slot per
// distinct commitment of f in first-use order, then H's h_i, the W_j of w and
// of zw, and g1 for e; qprog = (slot, eval) per query in set order.
constexpr uint32_t kAccNoPair = 0xffffffffu;  // a pair's missing second term
struct AccTerms {
  std::vector<uint32_t> termsrc;  // (kind << 28) | idx ; VK index space: fixed, sigma, g1
  std::vector<uint32_t> qprog;
  uint32_t nslots = 0, h_slot0 = 0, T = 0, Tp = 0;  // Tp: proof-point terms (the powers-table chains)
  // pairs of terms of one output for the one-lane form's two-term lanes
  // (k_acc_termmul NT = 2), per output range as k_acc_sum folds them
  std::vector<uint32_t> pairs;  // (t, t + 1 or kAccNoPair) per pair
  uint32_t npair = 0;
};
inline void acc_terms(const pm_proof_shape* s, const AccLayout& L, const std::vector<std::vector<AccQuery>>& sets,
                      AccTerms& t) {
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> slot_of;
  auto vk_index = [&](uint32_t kind, uint32_t idx) -> uint32_t {
    return kind == kRefFixed ? idx : s->num_fixed_columns + idx;
  };
  for (auto& st : sets)
    for (auto& x : st) {
      uint32_t slot = kSlotH;
      if (x.ref_kind != kRefH) {
        auto key = std::make_pair(x.ref_kind, x.ref_idx);
        auto it = slot_of.find(key);
        if (it == slot_of.end()) {
          slot = (uint32_t)t.termsrc.size();
          slot_of[key] = slot;
          t.termsrc.push_back(x.ref_kind == kRefProof ? x.ref_idx : ((1u << 28) | vk_index(x.ref_kind, x.ref_idx)));
        } else {
          slot = it->second;
        }
      }
      t.qprog.push_back(slot);
      t.qprog.push_back(x.eval);
    }
  t.h_slot0 = (uint32_t)t.termsrc.size();
  for (uint32_t i = 0; i < s->quotient_degree; i++) t.termsrc.push_back(L.p_h + i);
  t.nslots = (uint32_t)t.termsrc.size();
  for (uint32_t j = 0; j < L.nsets; j++) t.termsrc.push_back(L.p_W + j);  // w
  for (uint32_t j = 0; j < L.nsets; j++) t.termsrc.push_back(L.p_W + j);  // zw
  t.termsrc.push_back((1u << 28) | (s->num_fixed_columns + s->n_perm_columns));  // e: g1
  t.T = (uint32_t)t.termsrc.size();
  t.Tp = 0;
  for (uint32_t v : t.termsrc) t.Tp += (v >> 28) == 0 ? 1u : 0u;
  t.pairs.clear();
  t.npair = 0;
  {
    const uint32_t T0 = (uint32_t)t.termsrc.size(), ns = t.nslots, nst = L.nsets;
    const uint32_t lo[4] = {0, ns, ns + nst, T0 - 1}, hi[4] = {ns, ns + nst, ns + 2 * nst, T0};
    for (int o = 0; o < 4; o++)
      for (uint32_t k = lo[o]; k < hi[o]; k += 2) {
        t.pairs.push_back(k);
        t.pairs.push_back(k + 1 < hi[o] ? k + 1 : kAccNoPair);
        t.npair++;
      }
  }
}

// log2 of the lanes per term of the split (powers-table) form, 0 = the
// one-lane GLV form.  The powers tables pay only while their chains stay
// within ~3/4 of the lane budget: beyond it the 127-doubling chains share
// SIMDs and queue, while the one-lane GLV products still run in one pass at
// a flat ~1.16 ms.  Simple shape, T = 30 of which 21 proof points, wall per
// batch (profiles/r02/vkt/): split 1.13 ms at B = 1024, 1.67 at 1536 against
// one-lane 1.54 / 1.57 (the old rule without VK tables, 4 B T <= budget:
// profiles/r02/xover/).
// split: pm_ctx_set_accum_split (-1 = auto)
inline uint32_t acc_split_lanes(int split, size_t B, uint32_t T, uint32_t Tp) {
  const size_t nterm = B * T, nprf = B * Tp;
  uint32_t lgS = split >= 0 ? (uint32_t)split
                 : 4 * (nprf << 2) > 3 * kAccLaneBudget ? 0u
                                                        : acc_auto_lanes(nterm, 3);
  // 16 / 32 lanes per term only while the term additions still fit one wave
  // per SIMD (B = 16: k_acc_termadd 0.075 ms at 16 lanes, 0.061 at 32; B = 256
  // stays at 8 lanes: 0.129 ms, 16 lanes 0.138, 32 lanes 0.197:
  // profiles/r02/pow/timing_pow1.jsonl)
  if (split < 0 && lgS == 3)
    while (lgS < 5 && (nterm << (lgS + 1)) <= kAccLaneBudget / 2) lgS++;
  return lgS;
}

// The kernels' forms for a batch of B proofs of T terms (Tp of them proof
// points, npair two-term lanes).  The context's options come as plain ints,
// -1 = auto: split (pm_ctx_set_accum_split), tpl (PM_ACC_OPT_TERMS_PER_LANE),
// ladder (pm_ctx_set_accum_ladder: 0 quads, 1 row-sliced waves).
struct AccPathIn {
  size_t B;
  uint32_t T, Tp, npair;
  int split = -1, tpl = -1, ladder = -1;
  size_t nvk_build = 0;  // VK points whose powers tables this call builds beside the proofs' chains
  // k_acc_scalars: bytes of a proof's rows and of the tail (constants +
  // program), and the block's LDS cap; row_bytes = 0: np and lds are not asked
  size_t row_bytes = 0, tail_bytes = 0, lds_cap = 0;
};
struct AccPath {
  uint32_t lgS;     // log2 lanes per term of the split form, 0 = the one-lane GLV form
  bool quad_terms;  // k_acc_termadd<Cv, true>
  uint32_t lgT;     // log2 of lanes (or quads) per term
  int tpl;          // the one-lane form's terms per lane (0 in the split form)
  uint32_t pstep;   // k_acc_sum's row step (2 after two-term lanes)
  uint32_t lgL;     // log2 lanes per output of k_acc_sum
  bool sliced;      // the split form's ladder: row-sliced waves (else a quad per chain)
  uint32_t np;      // k_acc_scalars: proofs per block
  size_t lds;       // ... and its LDS request (the whole cap beside a split ladder: the fence)
};
inline AccPath acc_path(const AccPathIn& in) {
  AccPath p{};
  const size_t B = in.B, nterm = B * in.T, nprf = B * in.Tp;
  p.lgS = acc_split_lanes(in.split, B, in.T, in.Tp);
  // few terms (B <= ~34 for the simple shape): 16 quads per term with
  // quad-cooperative additions (k_acc_termadd<Cv, true>)
  p.quad_terms = in.split < 0 && p.lgS == 5 && nterm * 64 <= kAccLaneBudget / 2;
  p.lgT = p.quad_terms ? 4u : p.lgS;  // log2 of lanes (or quads) per term
  p.pstep = 1;
  if (p.lgS > 0) {
    // few chains: one row-sliced wave per chain (slice29.hpp, ~2x shorter
    // steps while the waves fit one per SIMD); more: a quad per chain
    const size_t chains = nprf + in.nvk_build;
    p.sliced = in.ladder >= 0 ? in.ladder == 1 : chains <= kAccSlicedChains;
  } else {
    // GLV products by signed 3-bit windows; two terms of one output per lane
    // (shared doublings) once one term per lane would put more than one wave
    // on a SIMD, while the pairs still fit one wave per SIMD (their 144 KiB of
    // LDS tables per block keep one block per CU); PM_ACC_OPT_TERMS_PER_LANE
    // forces 1 or 2
    const bool pairs_fit = (size_t)B * in.npair <= kAccLaneBudget / 2;
    p.tpl = in.tpl > 0 ? in.tpl : (nterm > kAccLaneBudget / 2 && pairs_fit ? 2 : 1);
    if (p.tpl == 2) p.pstep = 2;
  }
  // lanes per output: at most ~16 K in total.  The affine conversion runs on
  // lane 0 of each group, and it slowed from ~0.08 to ~0.14 ms when 32
  // lanes per output spread the 1024 outputs of B = 256 over 512 waves
  // (profiles/r01_s4/accum_sum_lanes.jsonl).
  uint32_t lgL = 0;
  while (lgL < 5 && ((size_t)B * 4 << (lgL + 1)) <= kAccSumLanes) lgL++;
  // large batches: still quads (quad-cooperative additions and inversion),
  // up to two per output, within one wave per SIMD; one lane per output ran
  // f's ~12 term sums and a lone-lane inversion while the w / zw / e lanes of
  // its wave idled (round 6, profiles/r06/sum_lanes_ab.jsonl: B = 4096 0.133
  // -> 0.114 ms, 3072 0.133 -> 0.080)
  while (lgL < 3 && ((size_t)B * 4 << (lgL + 1)) <= kAccLaneBudget / 2) lgL++;
  p.lgL = lgL;
  if (in.row_bytes) {
    // k_acc_scalars: 4 waves per block of np proofs (row_bytes / tail_bytes
    // above, checked against kAccScalarsLds before the first launch)
    // 16 proofs per block (round 5): wave 0 then runs the Lagrange chain with a
    // quad per proof (acc_lagrange_q, ~half the one-lane chain); more blocks
    // only spread the batch over more CUs
    p.np = (uint32_t)std::min<size_t>(16, (in.lds_cap - in.tail_bytes) / in.row_bytes - 1);
    p.lds = std::max(in.row_bytes * (p.np + 1) + in.tail_bytes, p.lgS > 0 ? in.lds_cap : 0);
  }
  return p;
}

}  // namespace pm
