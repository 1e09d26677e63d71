// mtgp_flatten_uniform.h -- the device flattener with row-uniform control flow.
//
// mtgp_flatten.h's flatten_tree walks one tree per lane with data-dependent control flow: in a
// wave whose lanes hold different trees every branch of the walk is executed for the union of
// the lanes (measured: an 8k-instruction kernel, ~300 us at C3).  Here all lanes step through
// the row indices together and every per-row decision is a select:
//   pass 1 (rows ascending, gp.py:366-376 order): resolve each row -- constant / variable /
//     operator, operand references, constant folding -- and size it (unfused length `len` for the
//     limits, fused length `flen`, Sethi-Ullman need and operand order) into an LDS table laid
//     out [row][lane] (a child lookup is a gather with one lane per bank: conflict-free);
//   pass 2 (rows descending: a parent's row index is above its children's): the postorder
//     position of every reachable node follows from its parent's (first child at the parent's
//     start, second child after the first's code, the node's own word after both), so each node
//     writes its own instruction word directly.  A leaf operand is folded into its parent's word
//     (the fused superinstruction forms, mtgp_flatten.h fuse_pair), so every non-leaf node owns
//     exactly one word.
// The output (program words, lengths, status) is the one flatten_tree produces, word for word
// (tests/test_gpu_build.py compares with the host flattener).  A tree in which one row is reached
// from two parents (a shared sub-DAG, only in arbitrary arrays) needs its subtree emitted twice:
// k_flatten's lane re-runs the serial flatten_tree, k_flatten_wave walks it with one lane
// (u_serial_walk below).
#pragma once
#include "mtgp_flatten.h"

namespace mtgp {

// one leaf operand: a constant or a data slot
struct ULeaf {
  bool isc;
  float v;
  uint32_t slot;
};

MTGP_INLINE MTGP_HD MtgpInstr u_instr(uint32_t op, uint32_t slot, float imm) {
  MtgpInstr x;
  x.op = op << MTGP_OP_SHIFT;
  x.imm = is_var_op(op) ? bits_to_f32(slot * MTGP_SLOT_BYTES) : imm;
  return x;
}

MTGP_INLINE MTGP_HD MtgpInstr u_load(const ULeaf& x, bool push) {
  return x.isc ? u_instr(push ? MTGP_OP_LDCP : MTGP_OP_LDC, 0, x.v) : u_instr(push ? MTGP_OP_LDVP : MTGP_OP_LDV, x.slot, 0.0f);
}

// Emitter::op_leaf: acc = f(acc, leaf) (rev 0) or f(leaf, acc) (rev 1)
MTGP_INLINE MTGP_HD MtgpInstr u_op_leaf(int fn, int rev, const ULeaf& x) {
  int base;
  switch (fn) {
    case MTGP_FN_ADD: base = 0; rev = 0; break;
    case MTGP_FN_SUB: base = 1; break;
    case MTGP_FN_MUL: base = 3; rev = 0; break;
    default: base = 4; break;  // DIV
  }
  const int idx = base + ((base == 1 || base == 4) ? rev : 0);
  return x.isc ? u_instr(fam_op(FK_C, idx), 0, x.v) : u_instr(fam_op(FK_V, idx), x.slot, 0.0f);
}

// Emitter::op_stack
MTGP_INLINE MTGP_HD MtgpInstr u_op_stack(int fn, int rev) {
  int idx;
  switch (fn) {
    case MTGP_FN_ADD: idx = 0; break;
    case MTGP_FN_SUB: idx = rev ? 2 : 1; break;
    case MTGP_FN_MUL: idx = 3; break;
    default: idx = rev ? 5 : 4; break;
  }
  return u_instr(fam_op(FK_S, idx), 0, 0.0f);
}

// packed row record: kind 2 | fn 4 | slot 8 | isconst 1 | afirst 1 | need 5 (bits, low to high)
MTGP_INLINE MTGP_HD uint32_t u_pack(uint32_t kind, uint32_t fn, uint32_t slot, uint32_t isc, uint32_t afirst,
                                    uint32_t need) {
  return kind | fn << 2 | slot << 6 | isc << 14 | afirst << 15 | need << 16;
}
MTGP_INLINE MTGP_HD uint32_t u_kind(uint32_t w) { return w & 3u; }
MTGP_INLINE MTGP_HD uint32_t u_fn(uint32_t w) { return (w >> 2) & 15u; }
MTGP_INLINE MTGP_HD uint32_t u_slot(uint32_t w) { return (w >> 6) & 255u; }
MTGP_INLINE MTGP_HD bool u_isc(uint32_t w) { return (w >> 14) & 1u; }
MTGP_INLINE MTGP_HD uint32_t u_afirst(uint32_t w) { return (w >> 15) & 1u; }
MTGP_INLINE MTGP_HD uint32_t u_need(uint32_t w) { return (w >> 16) & 31u; }

// a unary node over a leaf: its word(s) at pos (one fused word for sin / cos, else load + op)
MTGP_INLINE MTGP_HD int u_unary_leaf(int fn, const ULeaf& la, bool push, MtgpInstr* w) {
  const MtgpInstr un = u_instr(unary_op(fn), 0, 0.0f);
  if (unary_fuses(fn)) {
    fuse_pair(u_load(la, push), un, &w[0]);
    return 1;
  }
  w[0] = u_load(la, push);
  w[1] = un;
  return 2;
}
MTGP_INLINE MTGP_HD bool u_leaf(uint32_t w) { return u_isc(w) || u_kind(w) == K_VAR; }

// --------------------------------------------------------------------------------------
// The wave flattener's per-row core (k_flatten_wave: one lane per row).  `Tab` is one program's
// tables, indexed by row: w (u_pack record), len (unfused length low 16, saturated | fused length
// high 16), cv (folded constant), val (the original value column), pos (pass 2 link, below),
// flag.  The kernel keeps them in LDS; tests/test_flatten_core_host.py runs the same functions
// over plain arrays, row after row, against flatten_tree.

// operand row jj of row i: an evaluated row (its table entry) or, for jj >= i, the original value
// column (gp.py:366-369)
struct UOperand {
  uint32_t w;
  ULeaf lf;
  int len, flen;
  bool leaf;
};

template <class Tab>
MTGP_INLINE MTGP_HD UOperand u_operand(const Tab& S, int jj, int i) {
  UOperand o;
  if (jj < i) {
    o.w = S.w[jj];
    const uint32_t ln = S.len[jj];
    o.len = (int)(ln & 0xffffu);
    o.flen = (int)(ln >> 16);
    o.lf.isc = u_isc(o.w);
    o.lf.v = S.cv[jj];
    o.lf.slot = u_slot(o.w);
    o.leaf = u_leaf(o.w);
  } else {
    o.w = u_pack(K_CONST, 0, 0, 1, 1, 0);
    o.lf.isc = true;
    o.lf.v = S.val[jj];
    o.lf.slot = 0;
    o.len = o.flen = 1;
    o.leaf = true;
  }
  return o;
}

// pass 1: operator row i (function fn, operand rows ja, jb) once its operand rows < i are resolved
template <class Tab>
MTGP_INLINE MTGP_HD void u_resolve_op(Tab& S, int i, int fn, int ja, int jb) {
  const int ar = fn_arity(fn);
  uint32_t kind = ar == 1 ? K_UNARY : K_BINARY, isc = 1, afirst = 1, need = 0;
  int len = 1, flen = 1;
  float cv = 0.0f;
  const UOperand a = u_operand(S, ja, i);
  UOperand b;
  b.w = 0; b.lf.isc = true; b.lf.v = 0.0f; b.lf.slot = 0; b.len = b.flen = 1; b.leaf = true;
  if (ar == 2) b = u_operand(S, jb, i);
  if (a.lf.isc && b.lf.isc) {  // constant subtree: folded with the kernel's fp32 primitives
    cv = apply_fn(fn, a.lf.v, ar == 1 ? 0.0f : b.lf.v);
  } else {
    isc = 0;
    if (ar == 1) {
      if (a.leaf) { len = 2; flen = unary_fuses(fn) ? 1 : 2; }
      else { len = a.len + 1; flen = a.flen + 1; need = u_need(a.w); }
    } else if (a.leaf && b.leaf) {
      len = 2; flen = 1;
    } else if (b.leaf) {
      len = a.len + 1; flen = a.flen + 1; need = u_need(a.w);
    } else if (a.leaf) {
      len = b.len + 1; flen = b.flen + 1; need = u_need(b.w);
    } else {
      const uint32_t pa = u_need(a.w), qb = u_need(b.w);
      len = a.len + b.len + 1;
      flen = a.flen + b.flen + 1;
      if (pa >= qb) { afirst = 1; need = pa > qb + 1 ? pa : qb + 1; }
      else { afirst = 0; need = qb > pa + 1 ? qb : pa + 1; }
    }
  }
  S.w[i] = u_pack(kind, (uint32_t)fn, 0, isc, afirst, need > 31u ? 31u : need);
  S.len[i] = (uint32_t)(len > 65535 ? 65535 : len) | (uint32_t)(flen > 65535 ? 65535 : flen) << 16;
  S.cv[i] = cv;
}

// Pass 2 in closed form.  The code of a non-leaf node is [first operand subtree][second operand
// subtree][own word], so a node's first word is the sum, over its path to the root, of what lies
// in front of it inside its parent: 0 for the operand evaluated first, the first operand's fused
// length for the second.  A node pushes the accumulator iff some link of that path is a second
// operand (the first operand inherits its parent's push).  Every non-leaf row writes one link per
// non-leaf operand row (u_claim: parent row | offset << 8 | second << 24 in pos[operand], and
// bump(operand) counts the claims); after that each row adds up its own path (u_walk), with no
// synchronisation between the levels.  A row claimed twice needs its code twice: u_serial_walk.
constexpr uint32_t kULinkNone = 0xffffffffu;
MTGP_INLINE MTGP_HD uint32_t u_link(int row, int off, bool second) {
  return (uint32_t)row | (uint32_t)off << 8 | (second ? 1u << 24 : 0u);
}
static_assert(MTGP_MAX_NODES <= 256, "u_link holds a row in 8 bits");

template <class Tab, class Bump>
MTGP_INLINE MTGP_HD void u_claim(Tab& S, int i, int ca, int cb, Bump bump) {
  const uint32_t w = S.w[i];  // (the caller passes non-leaf rows only: an operator, not folded)
  auto claim = [&](int c, int off, bool second) {
    S.pos[c] = u_link(i, off, second);
    bump(c);
  };
  const UOperand a = u_operand(S, ca, i);
  if (u_kind(w) == K_UNARY) {
    if (!a.leaf) claim(ca, 0, false);
    return;
  }
  const UOperand b = u_operand(S, cb, i);
  if (a.leaf && b.leaf) return;
  if (b.leaf) claim(ca, 0, false);
  else if (a.leaf) claim(cb, 0, false);
  else {
    const bool af = u_afirst(w) != 0;
    claim(af ? ca : cb, 0, false);
    claim(af ? cb : ca, af ? a.flen : b.flen, true);
  }
}

// first word of row i's code | push << 16, or -1 if the root does not reach row i.  A link points
// to a higher row, so the path ends.
template <class Tab>
MTGP_INLINE MTGP_HD int u_walk(const Tab& S, int i, int root) {
  int pos = 0;
  uint32_t push = 0;
  for (int cur = i; cur != root;) {
    const uint32_t e = S.pos[cur];
    if (e == kULinkNone) return -1;
    pos += (int)((e >> 8) & 0xffffu);
    push |= e >> 24;
    cur = (int)(e & 255u);
  }
  return pos | (int)(push << 16);
}

// the word(s) of non-leaf row i (operand rows ca, cb) whose code starts at pos: emit(at, word);
// visit(row, pos, push) names its non-leaf operand rows and where their code starts
template <class Tab, class Emit, class Visit>
MTGP_INLINE MTGP_HD void u_emit_node(const Tab& S, int i, int ca, int cb, int pos, bool push, Emit emit,
                                     Visit visit) {
  const uint32_t w = S.w[i];
  const int fn = (int)u_fn(w);
  const UOperand a = u_operand(S, ca, i);
  if (u_kind(w) == K_UNARY) {
    if (a.leaf) {
      MtgpInstr w2[2];
      const int nw = u_unary_leaf(fn, a.lf, push, w2);
      emit(pos, w2[0]);  // (nw is 1 or 2; no dynamic index into w2, which would put it in scratch)
      if (nw > 1) emit(pos + 1, w2[1]);
    } else {
      visit(ca, pos, push);
      emit(pos + a.flen, u_instr(unary_op(fn), 0, 0.0f));
    }
    return;
  }
  const UOperand b = u_operand(S, cb, i);
  if (a.leaf && b.leaf) {
    MtgpInstr x;
    fuse_pair(u_load(a.lf, push), u_op_leaf(fn, 0, b.lf), &x);
    emit(pos, x);
  } else if (b.leaf) {
    visit(ca, pos, push);
    emit(pos + a.flen, u_op_leaf(fn, 0, b.lf));
  } else if (a.leaf) {
    visit(cb, pos, push);
    emit(pos + b.flen, u_op_leaf(fn, 1, a.lf));
  } else {
    const bool af = u_afirst(w) != 0;
    const int f1 = af ? a.flen : b.flen, f2 = af ? b.flen : a.flen;
    visit(af ? ca : cb, pos, push);
    visit(af ? cb : ca, pos + f1, true);
    emit(pos + f1 + f2, u_op_stack(fn, af ? 1 : 0));
  }
}

// The same words for a tree in which a row has two parents (arbitrary arrays only): one caller
// walks from the root with a stack of (row, pos, push) frames kept in pos[0 .. stack_cap), so a
// shared row is emitted once per path, as flatten_tree's emit_program does.  The lengths of pass 1
// already count it once per path, so the positions are the closed form above.  The stack holds at
// most one waiting operand per level and a level's row index is below its parent's: <= N frames.
// kids(row, ca, cb) gives a row's operand rows.  Returns false after more than `cap` nodes (cannot
// happen while the root's unfused length is <= cap; the bound keeps a broken table from looping).
template <class Tab, class Emit, class Kids>
MTGP_INLINE MTGP_HD bool u_serial_walk(Tab& S, int root, int cap, int stack_cap, Emit emit, Kids kids) {
  int top = 0, seen = 0;
  S.pos[0] = u_link(root, 0, false);
  while (top >= 0) {
    const uint32_t e = S.pos[top--];
    if (++seen > cap) return false;
    const int i = (int)(e & 255u);
    int ca = 0, cb = 0;
    kids(i, ca, cb);
    u_emit_node(S, i, ca, cb, (int)((e >> 8) & 0xffffu), (e >> 24) != 0u, emit, [&](int c, int cpos, bool cpush) {
      if (top + 1 < stack_cap) S.pos[++top] = u_link(c, cpos, cpush);
    });
  }
  return true;
}

// per-lane bit set over NMAX rows kept in registers (selects, never a dynamic index)
template <int NMAX>
struct UBits {
  static constexpr int W = (NMAX + 63) / 64;
  uint64_t w[W];
  MTGP_HD void clear() {
    for (int k = 0; k < W; ++k) w[k] = 0;
  }
  MTGP_HD bool test(int i) const {
    uint64_t r = 0;
    for (int k = 0; k < W; ++k) r = (k == (i >> 6)) ? w[k] : r;
    return (r >> (i & 63)) & 1ull;
  }
  MTGP_HD void set(int i) {
    for (int k = 0; k < W; ++k) w[k] |= (k == (i >> 6)) ? (1ull << (i & 63)) : 0ull;
  }
};

}  // namespace mtgp
