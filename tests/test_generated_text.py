"""CPU tier: an interpreter for the generated DPP text, at every dimension.

demcz_pw_wdpp_<D>.inc (the whitening of window_kernel_pw's log-density), demcz_pw_ddpp_<D>.inc (its candidate adds; D = 2..5:
the same text for window_kernel_ps2's switch) and demcz_ml_lrdpp_<D>.inc (the regression residuals on sixteen lanes per chain)
are asm blocks of v_fmac_f64_dpp with row_newbcast.  scripts/gen_*.py --check (tests/test_abi.py) proves the files are what the
generators write; this file proves that what they write computes the right doubles: every asm block is parsed as text, each %N
/ %[name] resolved through the block's own operand lists to the C++ expression it names, and the instructions are executed on a
model of a 64-lane wave -- dst[l] = fma(src0[16 (l / 16) + L], src1[l], dst[l]) for the lanes in EXEC, one rounding
(helpers.py_fma).  The lane-packed inputs are filled by the contract the kernels' comments state (demcz_kernels_pw.h,
demcz_kernels_ml.h), written here on its own: nothing is imported from scripts/.  Bit equality throughout."""
import re
from pathlib import Path

import numpy as np
import pytest

from helpers import bits_differ, py_fma

CSRC = Path(__file__).resolve().parent.parent / "demc.jl_amd" / "csrc"
LANES, ROW = 64, 16
FULL = (1 << LANES) - 1
PASS = 5


# ---- the text ---------------------------------------------------------------------------------------------------------------------
def _split_asm(body):
    """The parts of asm(...) between its top-level colons: [template, outputs, inputs, clobbers...]; string literals kept whole."""
    parts, cur, depth, i = [], "", 0, 0
    while i < len(body):
        ch = body[i]
        if ch == '"':
            j = i + 1
            while body[j] != '"':
                j += 2 if body[j] == "\\" else 1
            cur += body[i:j + 1]
            i = j + 1
            continue
        if ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
        if ch == ":" and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
        i += 1
    return parts + [cur]


_OPERAND = re.compile(r'(?:\[(\w+)\]\s*)?"([^"]*)"\s*\(([^()]+)\)')


def parse_blocks(text):
    """[(statements before the asm, instructions, operands, statements behind it)] of every `{ ... asm(...); ... }` block.
    operands: {"0": ("+v", "acc0"), ..., "name": (constraint, expression)} -- positions count outputs first, then inputs."""
    blocks = []
    for m in re.finditer(r"^\{(.*?)asm(?: volatile)?\((.*?)\);(.*?)\}$", text, flags=re.S | re.M):
        parts = _split_asm(m.group(2))
        assert len(parts) >= 3, "asm block without operand lists"
        template = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', parts[0])).replace("\\n", "\n").replace("\\t", "\t")
        operands, n = {}, 0
        for part in parts[1:3]:
            for name, constraint, expr in _OPERAND.findall(part):
                operands[str(n)] = (constraint, expr.strip())
                if name:
                    operands[name] = (constraint, expr.strip())
                n += 1
        instructions = [ln.strip() for ln in template.split("\n") if ln.strip()]
        blocks.append((m.group(1).strip(), instructions, operands, m.group(3).strip()))
    return blocks


# ---- the wave ---------------------------------------------------------------------------------------------------------------------
class Wave:
    """Vector registers by the C++ expression that names them (64 doubles each), scalar registers likewise, EXEC."""

    def __init__(self):
        self.v, self.s, self.exec = {}, {}, FULL
        self.disabled_sources = []        # (instruction, lane, source lane): a DPP read of a lane that EXEC has switched off
        self.fmas = 0

    def _name(self, token, operands, want):
        m = re.fullmatch(r"%(\d+)|%\[(\w+)\]", token)
        assert m, f"operand {token!r}"
        constraint, expr = operands[m.group(1) or m.group(2)]
        assert want in constraint, f"{token} names {expr} with constraint {constraint!r}, used as a {want} register"
        return constraint, expr

    def run(self, instructions, operands):
        for ins in instructions:
            op, _, rest = ins.partition(" ")
            if op == "s_nop":
                assert re.fullmatch(r"\d+", rest)
            elif op == "s_mov_b64":
                dst, src = [t.strip() for t in rest.split(",")]
                if dst == "exec":
                    self.exec = self.s[self._name(src, operands, "s")[1]]
                else:
                    assert src == "exec"
                    constraint, expr = self._name(dst, operands, "s")
                    assert "=" in constraint
                    self.s[expr] = self.exec
            elif op == "s_and_b64":
                dst, a, b = [t.strip() for t in rest.split(",")]
                assert dst == "exec" and a == "exec"
                self.exec &= self.s[self._name(b, operands, "s")[1]]
            elif op == "v_fmac_f64_dpp":
                m = re.fullmatch(r"(\S+), (\S+), (\S+) row_newbcast:(\d+) row_mask:0xf bank_mask:0xf", rest)
                assert m, ins
                (cd, dst), (_, src0), (_, src1) = (self._name(t, operands, "v") for t in m.group(1, 2, 3))
                assert "+" in cd, f"{dst} is read and written: its constraint must say so"
                L = int(m.group(4))
                assert 0 <= L < ROW
                a, b, c = self.v[src0], self.v[src1], self.v[dst]
                new = list(c)
                for l in range(LANES):
                    if (self.exec >> l) & 1:
                        sl = ROW * (l // ROW) + L
                        if not (self.exec >> sl) & 1:
                            self.disabled_sources.append((ins, l, sl))       # (the hardware leaves the lane as it was)
                            continue
                        new[l] = py_fma(a[sl], b[l], c[l])
                        self.fmas += 1
                self.v[dst] = new
            else:
                raise AssertionError(f"instruction the interpreter does not know: {ins}")


def _values(rng, shape):
    """Random doubles of mixed magnitudes with zeros and -0.0 among them."""
    a = rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, size=max(2, flat.size // 7), replace=False)
    flat[idx[::2]] = 0.0
    flat[idx[1::2]] = -0.0
    return a


def test_py_fma_is_one_rounding():
    """The interpreter's arithmetic is a fused multiply-add: a product whose low half decides the result."""
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30              # a b = 1 - 2^-60 exactly
    assert py_fma(a, b, -1.0) == -2.0 ** -60 and a * b - 1.0 == 0.0
    assert str(py_fma(-0.0, 3.0, -0.0)) == "-0.0" and str(py_fma(0.0, 3.0, -0.0)) == "0.0"


def test_every_generated_file_is_interpreted_here():
    """The parametrised ranges below are the files that exist (a new dimension's text would otherwise go unread)."""
    found = {kind: sorted(int(re.search(r"_(\d+)\.inc$", p.name).group(1)) for p in CSRC.glob(f"demcz_{kind}_*.inc") if "sel" not in p.name)
             for kind in ("pw_wdpp", "pw_ddpp", "ml_lrdpp")}
    assert found == {"pw_wdpp": list(range(6, 33)), "pw_ddpp": list(range(2, 33)), "ml_lrdpp": list(range(2, 29))}


# ---- the whitening ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", range(6, 33))
def test_whitening_text_gives_the_oracles_q(oracle, D):
    """q of every lane = the q of target_logp's order -- row i's chain W_i0 r_0, fma by fma in j; q the rows in order -- on
    random r (a vector per lane) and W.  Contract (demcz_kernels_pw.h): W packed lower-triangular, entry e = i (i + 1) / 2 + j in
    lane e % 16 of every 16-lane row of Wr[e / 16]."""
    rng = np.random.default_rng(1000 + D)
    W = np.tril(_values(rng, (D, D)))
    r = _values(rng, (LANES, D))
    wave = Wave()
    for j in range(D):
        wave.v[f"rr[{j}]"] = [float(v) for v in r[:, j]]
    packed = [float(W[i, j]) for i in range(D) for j in range(i + 1)]
    nwr = -(-len(packed) // ROW)
    for k in range(nwr):
        wave.v[f"Wr[{k}]"] = [packed[ROW * k + l % ROW] if ROW * k + l % ROW < len(packed) else float("nan") for l in range(LANES)]
    q = None
    blocks = parse_blocks((CSRC / f"demcz_pw_wdpp_{D}.inc").read_text())
    for before, instructions, operands, behind in blocks:
        names = re.findall(r"double (\w+) = -0\.0;", before)
        assert re.sub(r"double \w+ = -0\.0;\s*", "", before) == "" and names
        for n in names:
            wave.v[n] = [-0.0] * LANES
        assert all(c == "v" for k, (c, e) in operands.items() if not e.startswith("acc")), "inputs are read only"
        wave.run(instructions, operands)
        for st in [s.strip() for s in behind.split(";") if s.strip()]:
            m1, m2 = re.fullmatch(r"q = (\w+) \* \1", st), re.fullmatch(r"q = fma\((\w+), \1, q\)", st)
            assert m1 or m2, st
            acc = wave.v[(m1 or m2).group(1)]
            q = [acc[l] * acc[l] for l in range(LANES)] if m1 else [py_fma(acc[l], acc[l], q[l]) for l in range(LANES)]
    assert wave.exec == FULL and not wave.disabled_sources and wave.fmas == LANES * D * (D + 1) // 2
    # the order written out ...
    ref = np.zeros(LANES)
    for l in range(LANES):
        for i in range(D):
            acc = float(W[i, 0]) * float(r[l, 0])
            for j in range(1, i + 1):
                acc = py_fma(float(W[i, j]), float(r[l, j]), acc)
            ref[l] = acc * acc if i == 0 else py_fma(acc, acc, ref[l])
    assert bits_differ(np.array(q), ref) is None, bits_differ(np.array(q), ref)
    # ... and the oracle's own: logp = fma(-0.5, q, c0) with mu = 0, c0 = 0 is -q / 2, exactly
    prob = oracle.Problem(LANES, D, 10, LANES, np.ones(D), 1, target=dict(kind="mvnormal", mu=np.zeros(D), W=W, c0=0.0))
    assert np.array_equal(-0.5 * np.array(q), oracle.logp(prob, r))


# ---- the candidate adds -----------------------------------------------------------------------------------------------------------
def _takes(lane, j):
    """Does this lane's node take generation j (1..5) of a pass?  Lane n = node n of the tree for n = 1..31 (level = bit length;
    below its level's first bit the bits are the accepts of generations 1..level - 1, the node's own proposal is made at
    generation `level`), lane 0 is the state, lanes 32..63 repeat node 1 (demcz_kernels_pw.h, `tk`)."""
    if lane == 0:
        return False
    n = lane if lane < 32 else 1
    level = n.bit_length()
    return j == level or (j < level and bool((n >> (level - 1 - j)) & 1))


def _common_positions(j):
    """Positions of a 16-lane row that take generation j in every row that has a taker, ascending (demcz_kernels_pw.h, `common`)."""
    rows = [{p for p in range(ROW) if _takes(ROW * r + p, j)} for r in range(LANES // ROW)]
    return sorted(set.intersection(*[s for s in rows if s]))


def test_common_positions_are_what_the_kernel_counts_on():
    assert [len(_common_positions(j)) for j in range(1, 6)] == [4, 4, 4, 4, 16]        # DD_KN, demcz_kernels_pw.h


@pytest.mark.parametrize("D", range(2, 33))
def test_candidate_add_text_builds_every_nodes_candidate(D):
    """Every node's candidate = the state plus the increments of the generations on its path, added in generation order; lane 0
    (the state) untouched; every DPP source lane switched on under its generation's EXEC.  Contract: generation u's D increments
    in ceil(D / KN) register pairs, entry q KN + m in the m-th common position of every row of Dg[u][q] (lanes elsewhere hold
    entry q KN, as the kernel's pointer arithmetic gives them, and must never be read)."""
    rng = np.random.default_rng(2000 + D)
    state = _values(rng, D)
    inc = _values(rng, (PASS, D))
    wave = Wave()
    for p in range(D):
        wave.v[f"cand[{p}]"] = [float(state[p])] * LANES
    wave.v["one"] = [1.0] * LANES
    for u in range(PASS):
        common = _common_positions(u + 1)
        kn = len(common)
        wave.s[f"tmask[{u}]"] = sum(1 << l for l in range(LANES) if _takes(l, u + 1))
        for qq in range(-(-D // kn)):
            reg = []
            for l in range(LANES):
                pos = l % ROW
                e = qq * kn + (common.index(pos) if pos in common else 0)
                # (a poisoned value wherever the contract puts nothing that may be read: the padding, the positions not common)
                reg.append(float(inc[u, e]) if e < D and pos in common else float("nan"))
            wave.v[f"Dg[{u}][{qq}]"] = reg
    blocks = parse_blocks((CSRC / f"demcz_pw_ddpp_{D}.inc").read_text())
    assert len(blocks) == PASS
    for u, (before, instructions, operands, behind) in enumerate(blocks):
        assert "uint64_t sv;" in before and behind == ""
        assert operands["mask"] == ("s", f"tmask[{u}]") and operands["one"] == ("v", "one") and operands["sv"] == ("=&s", "sv")
        assert instructions[0] == "s_mov_b64 %[sv], exec" and instructions[-1] == "s_mov_b64 exec, %[sv]"
        nfma = wave.fmas
        wave.run(instructions, operands)
        assert wave.exec == FULL, "EXEC restored"
        assert wave.fmas - nfma == D * bin(wave.s[f"tmask[{u}]"]).count("1")
    assert not wave.disabled_sources, wave.disabled_sources[:3]
    got = np.array([wave.v[f"cand[{p}]"] for p in range(D)]).T          # (lane, parameter)
    ref = np.empty((LANES, D))
    for l in range(LANES):
        x = [float(v) for v in state]
        for j in range(1, PASS + 1):
            if _takes(l, j):
                x = [x[p] + float(inc[j - 1, p]) for p in range(D)]
        ref[l] = x
    assert bits_differ(got[0], state) is None, "lane 0 keeps the state"
    assert bits_differ(got, ref) is None, bits_differ(got, ref)
    assert not np.isnan(got).any()


# ---- the regression residuals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", range(2, 29))
def test_regression_text_gives_target_logps_products(D):
    """a_g of every lane (an observation each) = x_o0 b_0, then fma by fma in j, for each of the wave's four chains g.  Contract
    (demcz_kernels_ml.h): proposal entry e = g D + j in lane e % 16 of every 16-lane row of Bp[e / 16]; rowv[j] the lane's design
    row; a0..a3 start as -0.0."""
    NG = 4
    rng = np.random.default_rng(3000 + D)
    design = _values(rng, (LANES, D))
    b = _values(rng, (NG, D))
    wave = Wave()
    for j in range(D):
        wave.v[f"rowv[{j}]"] = [float(v) for v in design[:, j]]
    flat = [float(v) for v in b.reshape(-1)]
    for k in range(-(-len(flat) // ROW)):
        wave.v[f"Bp[{k}]"] = [flat[ROW * k + l % ROW] if ROW * k + l % ROW < len(flat) else float("nan") for l in range(LANES)]
    for g in range(NG):
        wave.v[f"a{g}"] = [-0.0] * LANES
    for before, instructions, operands, behind in parse_blocks((CSRC / f"demcz_ml_lrdpp_{D}.inc").read_text()):
        assert before == "" and behind == ""
        assert all(c == "v" for k, (c, e) in operands.items() if not re.fullmatch(r"a\d", e)), "inputs are read only"
        wave.run(instructions, operands)
    assert wave.exec == FULL and not wave.disabled_sources and wave.fmas == LANES * NG * D
    got = np.array([wave.v[f"a{g}"] for g in range(NG)])
    ref = np.empty((NG, LANES))
    for g in range(NG):
        for o in range(LANES):
            acc = float(design[o, 0]) * float(b[g, 0])
            for j in range(1, D):
                acc = py_fma(float(design[o, j]), float(b[g, j]), acc)
            ref[g, o] = acc
    assert bits_differ(got, ref) is None, bits_differ(got, ref)
