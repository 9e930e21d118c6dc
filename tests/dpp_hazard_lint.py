"""DPP read hazards in a disassembly listing (llvm-objdump -d --mcpu=gfx950 --symbolize-operands), as a function over text.

gfx9-family hardware does not interlock a DPP read against the vector ALU: software keeps two wait states between a vector-ALU write
of a VGPR and a DPP read of it, and five between a vector-ALU write of EXEC and any DPP instruction (the constants of LLVM's
GCNHazardRecognizer::checkDPPHazards; csrc/tmpc_wave.hpp states the first).  The compiler's hazard recognizer places the waits
for the instructions it emits and does not look into inline assembly, which is where csrc/tmpc_wave.hpp issues its
v_fmac_f64_dpp / v_mov_b64_dpp.

The lint looks at DPP controls, `s_nop` and the destinations of `v_*` instructions, and at nothing else.  For every instruction with
a DPP control it walks back until the wait states are covered: an instruction counts 1, `s_nop N` counts N + 1.  A window that
reaches a label or a branch ends there (other paths into or out of the block are not followed) and is counted as cut."""
import re

VGPR_WAIT, EXEC_WAIT = 2, 5

_LABEL = re.compile(r"^[0-9a-fA-F]+ <[^>]*>:\s*$|^[A-Za-z_.$][\w.$]*:\s*$")
_DPP_CTRL = re.compile(r"\b(quad_perm:|row_shl:|row_shr:|row_ror:|wave_shl|wave_shr|wave_rol|wave_ror|row_mirror|row_half_mirror|"
                       r"row_bcast:|row_newbcast:|row_share:|row_xmask:|dpp8:)")
_REG = re.compile(r"^([va])(\d+)$|^([va])\[(\d+):(\d+)\]$")
_BRANCH = re.compile(r"^s_(c?branch|setpc|swappc|call|endpgm|trap|rfe)")
_WRITES_ALL = re.compile(r"^v_(swap_|permlane\d+_swap)")      # both operands are destinations


def _operands(rest):
    """comma-separated operands; brackets keep their commas (v[4:5], quad_perm:[1,0,3,2])"""
    out, depth, cur = [], 0, ""
    for ch in rest:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _regs(op):
    """{(file, index)} of a register operand `v4`, `v[4:5]`, `a3`, `|v[2:3]|`, `-v1`; empty for anything else"""
    op = op.strip().strip("|").lstrip("-").strip("|")
    m = _REG.match(op)
    if not m:
        return set()
    if m.group(1):
        return {(m.group(1), int(m.group(2)))}
    return {(m.group(3), i) for i in range(int(m.group(4)), int(m.group(5)) + 1)}


_INS = re.compile(r"^[a-z_][a-z0-9_]*(\s|$)")


def parse_line(no, raw):
    """("label",), ("ins", line number, mnemonic, operands, source text), or None for a line that is neither"""
    body = raw.split("//")[0].strip()
    if not body:
        return None
    if _LABEL.match(body):
        return ("label",)
    if not _INS.match(body):
        return None          # section headers, file format lines, data
    parts = body.split(None, 1)
    rest = parts[1] if len(parts) > 1 else ""
    # (modifiers follow the last operand after a blank: `v4 quad_perm:[1,0,3,2] row_mask:0xf`)
    return ("ins", no, parts[0], [o.split()[0] for o in _operands(rest)], body)


def _is_dpp(it):
    return it[2].startswith("v_") and ("_dpp" in it[2] or _DPP_CTRL.search(it[4]) is not None)


def _valu_writes(it):
    """VGPRs / AGPRs a vector-ALU instruction writes (MFMA included)"""
    mnem, ops = it[2], it[3]
    if not mnem.startswith("v_") or not ops:
        return set()
    if _WRITES_ALL.match(mnem):
        return set().union(*[_regs(o) for o in ops])
    return _regs(ops[0])


def lint(text):
    """-> dict(dpp=number of DPP instructions, cut=windows that ended at a label or a branch,
               violations=[(line number, DPP instruction, line number, offending instruction, wait states between)])"""
    lines = text.split("\n")
    cache = {}

    def item(i):      # (parsed on demand: a listing of the product has 1.3 million lines, 2 % of them near a DPP read)
        if i not in cache:
            cache[i] = parse_line(i + 1, lines[i])
        return cache[i]

    n_dpp = n_cut = 0
    bad = []
    for at, raw in enumerate(lines):
        if "_dpp" not in raw and _DPP_CTRL.search(raw) is None:
            continue
        it = item(at)
        if it is None or it[0] != "ins" or not _is_dpp(it):
            continue
        n_dpp += 1
        src = _regs(it[3][1]) if len(it[3]) > 1 else set()
        covered, k, cut = 0, at, False
        while covered < EXEC_WAIT:
            k -= 1
            if k < 0:
                break
            p = item(k)
            if p is None:
                continue
            if p[0] == "label" or _BRANCH.match(p[2]):
                cut = True
                break
            if covered < VGPR_WAIT and src & _valu_writes(p):
                bad.append((it[1], it[4], p[1], p[4], covered))
            if p[2].startswith("v_cmpx"):
                bad.append((it[1], it[4], p[1], p[4], covered))
            if p[2] == "s_nop":
                covered += int(p[3][0], 0) + 1
            else:
                covered += 1
        n_cut += cut
    return {"dpp": n_dpp, "cut": n_cut, "violations": bad}
