"""What the instruction-stream generators (gen_gemm_w4.py, gen_attn_fwd.py, gen_attn_dq.py, gen_attn_dkv.py) have in common: the
text model of an instruction list (register names, issue cost, operands, counted LDS waits, MFMAs placed with their gaps), the
lane-constant address set-up of the d = 128 attention kernels, the writer of the generated header and the command line.
An instruction is a string, a label a string that ends in ':'; every emitter below returns a list of them and is parametrised by
the registers it writes (numbers; V / A / S name them).  tools/cdna_emu.py, which checks the generators, shares nothing with this."""
import os
import re
import sys


def V(b, n=1):
    return "v%d" % b if n == 1 else "v[%d:%d]" % (b, b + n - 1)


def A(b, n=1):
    return "a%d" % b if n == 1 else "a[%d:%d]" % (b, b + n - 1)


def S(b, n=1):
    return "s%d" % b if n == 1 else "s[%d:%d]" % (b, b + n - 1)


def mfma32(d, a, b, c):
    return "v_mfma_f32_32x32x16_bf16 %s, %s, %s, %s" % (d, a, b, c)


COST = {"v_exp_f32": 8, "v_mul_lo_u32": 8, "v_log_f32": 8, "v_rcp_f32": 8}


def cost(text):
    op = text.split()[0]
    if op.startswith("ds_") or op.startswith("s_"):
        return 1
    return COST.get(op, 4)


class Fixed(dict):
    """{gap: [instructions]}: what a phase pins to an MFMA gap (reads, barriers, LDS-DMA pieces)"""
    def add(self, g, ins):
        self.setdefault(g, []).extend(ins if isinstance(ins, list) else [ins])


def place(mf, gaps, fixed):
    """mf: MFMA texts; gaps: one instruction list per MFMA gap (may be shorter than mf); fixed: {gap: [instructions]}, which go
    first in their gap -> flat list"""
    out = []
    for m, ins in enumerate(mf):
        out.append(ins)
        out += fixed.get(m, [])
        if m < len(gaps):
            out += gaps[m]
    return out


# ---- counted LDS waits ---------------------------------------------------------------------------------------------------
def regs_of(tok):
    """registers named by an operand token -> set of ('v' | 'a' | 's', index)"""
    tok = tok.strip()
    out = set()
    if not tok or tok[0] not in "vas" or tok in ("vcc", "scc", "s_nop"):
        return out
    kind = tok[0]
    body = tok[1:]
    if body.startswith("["):
        lo, hi = body[1:-1].split(":")
        for r in range(int(lo), int(hi) + 1):
            out.add((kind, r))
    elif body.isdigit():
        out.add((kind, int(body)))
    return out


def operands(text):
    parts = text.split(None, 1)
    if len(parts) < 2:
        return parts[0], []
    ops = [x.strip() for x in parts[1].split(",")]
    last = ops[-1].split()
    if last:
        ops[-1] = last[0]
    return parts[0], ops


def insert_lgkm_waits(seq, carry=()):
    """seq: flat instruction list entered with the LDS reads `carry` (destination-register sets, oldest first) outstanding.  Inserts the minimal counted s_waitcnt lgkmcnt(n) in front of every instruction that
    touches a register an outstanding LDS read will still write (reads return in issue order; counts above 15 clamp)."""
    out, pend = [], [set(x) for x in carry]          # pend: list of destination-register sets, oldest first
    for ins in seq:
        op, ops = operands(ins)
        if op == "s_waitcnt":
            if "lgkmcnt(0)" in ins:
                pend = []
            out.append(ins)
            continue
        if op.endswith(":"):
            out.append(ins)
            continue
        touched = set()
        for o in ops:
            touched |= regs_of(o)
        need = None
        for k, dst in enumerate(pend):
            if dst & touched:
                need = k
        if need is not None:
            n = len(pend) - 1 - need
            n = min(n, 15)
            out.append("s_waitcnt lgkmcnt(%d)" % n)
            pend = pend[len(pend) - n:] if n > 0 else []
        if op.startswith("ds_read"):
            pend.append(regs_of(ops[0]))
        elif op.startswith("ds_write"):
            pend.append(set())                      # an LDS store occupies a slot of the same counter
        out.append(ins)
    return out, pend


def to1616(lines):
    """TIMING ONLY (cfg abl_1616; results are garbage): every v_mfma_f32_32x32x16_bf16 becomes two v_mfma_f32_16x16x32_bf16 of the same
    FLOPs on the first eight registers of its accumulator block, same operand registers, same place in the stream, and the
    softmax guard never branches -- what this schedule would run at on the other MFMA shape (profiles/r04_attn_1616_probe.txt)"""
    out = []
    for l in lines:
        m = re.match(r"v_mfma_f32_32x32x16_bf16 ([av])\[(\d+):\d+\], (\S+), (\S+), (?:([av])\[(\d+):\d+\]|0)$", l)
        if m:
            dk, d0, a, b, ck = m.group(1), int(m.group(2)), m.group(3), m.group(4), m.group(5)
            for h in range(2):
                c = "0" if ck is None else "%s[%d:%d]" % (ck, int(m.group(6)) + 4 * h, int(m.group(6)) + 4 * h + 3)
                out.append("v_mfma_f32_16x16x32_bf16 %s[%d:%d], %s, %s, %s" % (dk, d0 + 4 * h, d0 + 4 * h + 3, a, b, c))
        elif l.startswith("v_mfma"):
            raise ValueError("to1616: " + l)
        elif l.startswith("s_cbranch_vccnz o2af_fix") or l.startswith("s_cbranch_vccnz o2dq_fix"):
            out.append("s_nop 0")
        else:
            out.append(l)
    return out


# ---- address set-up of the attention kernels --------------------------------------------------------------------------------
# LDS image of a 64-row x 128-column bf16 tile (16 KiB) = 8-row x 32-column subtiles of 512 B:
#   off(row, 16-byte chunk ch) = 2048 (row >> 3) + 512 (ch >> 2) + 64 (row & 7) + 16 ((ch & 3) ^ ((row >> 2) & 3))
# so every row read and every transposed read of a tile is a lane-constant address register plus an immediate.
def lane_id(lane):
    return ["v_mbcnt_lo_u32_b32 %s, -1, 0" % V(lane), "v_mbcnt_hi_u32_b32 %s, -1, %s" % (V(lane), V(lane))]


def row_read_base(lane, lds, r, h, t, even, odd, second=None):
    """bases of the ds_read_b128 row reads (an MFMA A / B fragment of row r, k-half h): v[r] <- r = lane & 31 and v[h] <- h = lane >> 5
    (both are left for the emitters below), v[even] <- %lds + 2048 (r >> 3) + 64 (r & 7) + 16 (h ^ ((r >> 2) & 3)), v[odd] <- even ^ 32
    for the odd k-steps; second = (even, odd) of the image 64 KiB up, where a kernel keeps its second operand."""
    L = ["v_and_b32 %s, 31, %s" % (V(r), V(lane)),
         "v_lshrrev_b32 %s, 5, %s" % (V(h), V(lane)),
         "v_lshrrev_b32 %s, 3, %s" % (V(t), V(r)),
         "v_lshlrev_b32 %s, 11, %s" % (V(even), V(t)),
         "v_and_b32 %s, 7, %s" % (V(t), V(r)),
         "v_lshl_add_u32 %s, %s, 6, %s" % (V(even), V(t), V(even)),
         "v_bfe_u32 %s, %s, 2, 2" % (V(t), V(r)),                       # (r >> 2) & 3
         "v_xor_b32 %s, %s, %s" % (V(t), V(t), V(h)),
         "v_lshl_add_u32 %s, %s, 4, %s" % (V(even), V(t), V(even)),
         "v_add_u32 %s, %s, %s" % (V(even), S(lds), V(even)),
         "v_xor_b32 %s, 32, %s" % (V(odd), V(even))]
    if second:
        L += ["v_add_u32 %s, 0x10000, %s" % (V(second[0]), V(even)), "v_add_u32 %s, 0x10000, %s" % (V(second[1]), V(odd))]
    return L


def tr_read_base(lane, lds, h, t, u, first, other, second=None):
    """bases of the ds_read_b64_tr_b16 transposed reads; v[h] = lane >> 5 on entry, v[t] / v[u] scratch.  With g1 = (lane >> 4) & 1,
    q = (lane & 15) >> 2, p = lane & 3: v[first] <- %lds + 64 (4 h + q) + 16 ((2 g1 + (p >> 1)) ^ h) + 8 (p & 1), v[other] <-
    (first ^ 32) + 2048 for the second block of a fragment; second = (first, other) of the image 64 KiB up."""
    L = ["v_bfe_u32 %s, %s, 2, 2" % (V(t), V(lane)),                      # q
         "v_lshl_add_u32 %s, %s, 2, %s" % (V(t), V(h), V(t)),             # 4 h + q
         "v_lshlrev_b32 %s, 6, %s" % (V(first), V(t)),
         "v_bfe_u32 %s, %s, 4, 1" % (V(t), V(lane)),                      # g1
         "v_bfe_u32 %s, %s, 1, 1" % (V(u), V(lane)),                      # p >> 1
         "v_lshl_add_u32 %s, %s, 1, %s" % (V(t), V(t), V(u)),             # 2 g1 + (p >> 1)
         "v_xor_b32 %s, %s, %s" % (V(t), V(t), V(h)),
         "v_lshl_add_u32 %s, %s, 4, %s" % (V(first), V(t), V(first)),
         "v_and_b32 %s, 1, %s" % (V(t), V(lane)),
         "v_lshl_add_u32 %s, %s, 3, %s" % (V(first), V(t), V(first)),
         "v_add_u32 %s, %s, %s" % (V(first), S(lds), V(first)),
         "v_xor_b32 %s, 32, %s" % (V(other), V(first)),
         "v_add_u32 %s, 0x800, %s" % (V(other), V(other))]
    if second:
        L += ["v_add_u32 %s, 0x10000, %s" % (V(second[0]), V(first)), "v_add_u32 %s, 0x10000, %s" % (V(second[1]), V(other))]
    return L


def dma_source_offsets(lane, h, t, u, even, odd, pitch):
    """per-lane global offsets of an LDS-DMA piece (8 rows x 64 columns, written to LDS in lane order, so the source is permuted
    into the image): v[even] <- ((lane >> 2) & 7) pitch + 16 (4 h + ((lane & 3) ^ ((lane >> 4) & 1))), v[odd] <- even ^ 32 for the
    pieces of the odd 8-row group (j >= 2, swizzle bit (row >> 3) & 1 set); pitch = the row pitch operand in bytes"""
    return ["v_bfe_u32 %s, %s, 2, 3" % (V(t), V(lane)),
            "v_mul_lo_u32 %s, %s, %s" % (V(even), V(t), pitch),
            "v_bfe_u32 %s, %s, 4, 1" % (V(t), V(lane)),
            "v_and_b32 %s, 3, %s" % (V(u), V(lane)),
            "v_xor_b32 %s, %s, %s" % (V(t), V(t), V(u)),
            "v_lshl_add_u32 %s, %s, 2, %s" % (V(t), V(h), V(t)),          # 4 h + x
            "v_lshl_add_u32 %s, %s, 4, %s" % (V(even), V(t), V(even)),
            "v_xor_b32 %s, 32, %s" % (V(odd), V(even))]


def kh_base(vkh, h, lds, off):
    """key-group hash table at LDS byte `off`: half h reads its 8 values of tile t at off + 64 t + 32 h"""
    return ["v_lshlrev_b32 %s, 5, %s" % (V(vkh), V(h)), "v_add_u32 %s, %s, %s" % (V(vkh), S(lds), V(vkh)),
            "v_add_u32 %s, 0x%x, %s" % (V(vkh), off, V(vkh))]


def kh_reads(kh, vkh):
    """the 8 key-group hashes of the next tile -> v[kh:kh+7]; the table pointer moves on"""
    return ["ds_read_b128 %s, %s" % (V(kh, 4), V(vkh)), "ds_read_b128 %s, %s offset:16" % (V(kh + 4, 4), V(vkh)),
            "v_add_u32 %s, 64, %s" % (V(vkh), V(vkh))]


def descriptor(sd, base, second=None):
    """raw buffer descriptor s[sd:sd+3]: base, stride 0, 2^31 - 1 bytes; second = (register, byte distance operand) of a further
    descriptor that far behind the first one's base"""
    L = ["s_mov_b64 %s, %s" % (S(sd, 2), base), "s_mov_b32 %s, 0x7fffffff" % S(sd + 2), "s_mov_b32 %s, 0x00020000" % S(sd + 3)]
    if second:
        s2, dist = second
        L += ["s_add_u32 %s, %s, %s" % (S(s2), S(sd), dist), "s_addc_u32 %s, %s, 0" % (S(s2 + 1), S(sd + 1)),
              "s_mov_b32 %s, 0x7fffffff" % S(s2 + 2), "s_mov_b32 %s, 0x00020000" % S(s2 + 3)]
    return L


def piece_offsets(pc, tmp, pitch):
    """s[pc + j] <- byte offset in a tile of piece j (0..3) of wave w: tile piece i = 4 w + j covers rows 8 (i >> 1) .., column
    half i & 1 -- pieces 0 / 1 the two halves of rows 16 w .., pieces 2 / 3 of rows 16 w + 8 .."""
    return ["s_lshl_b32 %s, %%[wave], 4" % S(tmp),                         # 16 w = 8 * (2 w)
            "s_mul_i32 %s, %s, %s" % (S(pc), S(tmp), pitch),
            "s_add_u32 %s, %s, 128" % (S(pc + 1), S(pc)),
            "s_lshl_b32 %s, %s, 3" % (S(tmp), pitch),
            "s_add_u32 %s, %s, %s" % (S(pc + 2), S(pc), S(tmp)),
            "s_add_u32 %s, %s, 128" % (S(pc + 3), S(pc + 2))]


def wave_lds_base(lw, lds, tmp):
    """s[lw] <- where this wave's 4 pieces (4 KiB) of a tile start in the tile's image"""
    return ["s_lshl_b32 %s, %%[wave], 12" % S(tmp), "s_add_u32 %s, %s, %s" % (S(lw), S(lds), S(tmp))]


def tile_offset(tmp, t, dt, last, outs):
    """for every (register, tile-bytes register) of outs: byte offset of tile min(t + dt, last); the tile index stays in s[tmp]"""
    return ["s_add_u32 %s, %s, %d" % (S(tmp), S(t), dt), "s_min_u32 %s, %s, %s" % (S(tmp), S(tmp), S(last))] + \
           ["s_mul_i32 %s, %s, %s" % (S(o), S(tmp), S(tb)) for o, tb in outs]


def dma_piece(desc, sof, spc, lw, dst, tmp, lane_offs):
    """one LDS-DMA piece (1 KiB: a wave's 64 lanes x 16 B): global offset s[tmp] = s[sof] (the tile) + s[spc] (the piece), LDS
    destination m0 = s[lw] + dst; lane_offs = the (even, odd) lane-offset registers' one that fits the piece"""
    return ["s_add_u32 %s, %s, %s" % (S(tmp), S(sof), S(spc)),
            "s_add_u32 m0, %s, %d" % (S(lw), dst),
            "s_nop 0",
            "buffer_load_dwordx4 %s, %s, %s offen lds" % (V(lane_offs), S(desc, 4), S(tmp))]


def frag_offset(off, r, h, t, pitch, with_h=True):
    """v[off] <- r pitch + 16 h: where lane (row r, k-half h) finds its 8 elements of k-step 0 in a row-major block; v[t] <- 16 h
    (with_h = False: v[t] holds it already)"""
    return (["v_lshlrev_b32 %s, 4, %s" % (V(t), V(h))] if with_h else []) + \
           ["v_mul_lo_u32 %s, %s, %s" % (V(off), V(r), pitch), "v_add_u32 %s, %s, %s" % (V(off), V(off), V(t))]


def frag_loads(dst, off, base):
    """the 8 k-step fragments of a 32-row block -> a[dst:dst+31]"""
    return ["global_load_dwordx4 %s, %s, %s offset:%d" % (A(dst + 4 * ds, 4), V(off), base, ds * 32) for ds in range(8)]


def block_frag_loads(x, y, off, ptr, sp, tmp, pitch):
    """8 + 8 fragment loads of a wave's 64 rows: block X at the pointer operand, block Y 32 rows on (pointer in s[sp:sp+1])"""
    return ["s_lshl_b32 %s, %s, 5" % (S(tmp), pitch),
            "s_mov_b64 %s, %s" % (S(sp, 2), ptr),
            "s_add_u32 %s, %s, %s" % (S(sp), S(sp), S(tmp)),
            "s_addc_u32 %s, %s, 0" % (S(sp + 1), S(sp + 1))] + frag_loads(x, off, ptr) + frag_loads(y, off, S(sp, 2))


# ---- the generated header and the command line -----------------------------------------------------------------------------
def emit(path, script, prefix, defines, macros, vregs, sregs, labels=True):
    """macros: [(name, instruction list)]; the clobber list names every accumulator register, v[vregs:255] and s[sregs[0]:sregs[1]-1].
    A label line ends in \\n, an instruction line in \\n\\t (labels = False: every line is written as an instruction)"""
    out = ["// GENERATED by tools/%s -- do not edit; the schedule lives in that script." % script, "#pragma once"] + defines
    for name, lines in macros:
        out.append("#define %s \\" % name)
        for k, s in enumerate(lines):
            end = "\\n" if labels and s.endswith(":") else "\\n\\t"
            out.append('  "%s%s"%s' % (s, end, " \\" if k + 1 < len(lines) else ""))
    clob = ['"memory"', '"scc"', '"vcc"'] + ['"a%d"' % r for r in range(256)] + ['"v%d"' % r for r in range(vregs, 256)] + \
           ['"s%d"' % r for r in range(*sregs)]
    out.append("#define %s_CLOBBERS \\" % prefix)
    for k in range(0, len(clob), 16):
        chunk = ", ".join(clob[k:k + 16])
        out.append("  %s%s" % (chunk, ", \\" if k + 16 < len(clob) else ""))
    open(path, "w").write("\n".join(out) + "\n")


def show(lines, mfmas=True):
    """the stream with the MFMA slot each instruction follows"""
    slot = -1
    for l in lines:
        if l.startswith("v_mfma"):
            slot += 1
            if not mfmas:
                continue
        print(slot, l)


def main(module, default_header):
    """`--cfg k=v,...` overrides module.BASE (a schedule parameter or a timing-only ablation), `show ...` prints the stream
    (module.show(arguments) where a generator has its own form, else gen(drop) unless `nodrop` is given), otherwise the header
    module.header() describes is written to csrc/ or to `--out PATH` (tools/mkvar_w4.sh, tools/mkvar_af.sh)"""
    argv = sys.argv
    if "--cfg" in argv:
        for kv in argv[argv.index("--cfg") + 1].split(","):
            k, v = kv.split("=")
            module.BASE[k] = int(v)
    if len(argv) > 1 and argv[1] == "show":
        if hasattr(module, "show"):
            module.show(argv[2:])
        else:
            show(module.gen("nodrop" not in argv))
    else:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(root, "orbit-2_amd", "csrc", default_header)
        emit(out, os.path.basename(module.__file__), **module.header())
        print("wrote %s" % out, module.BASE)
