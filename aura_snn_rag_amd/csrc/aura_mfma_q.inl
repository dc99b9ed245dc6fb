// aura_mfma_q.inl -- the two-stage scan's MFMA statement, hand-spaced inline asm.  Included by aura_knn_coarse.inl
// once per 16-bit operand format with AURA_MFMA_FN (the function's name) and AURA_MFMA_OP (the mnemonic, with a
// trailing blank) defined: v_mfma_f32_16x16x32_bf16 and v_mfma_f32_16x16x32_f16 share shape, register layout, pass
// count and hazards, so the two functions differ in the mnemonic alone.  No include guard on purpose.
template <bool QA, bool LAST, bool PAD, bool COND = false>
__device__ __forceinline__ void AURA_MFMA_FN(f32x4v& acc, const bf16x8v& af, const bf16x8v& q, int on = 1) {
    // COND: the MFMA runs only when `on` (wave-uniform, in an SGPR) is non-zero -- a scalar compare and
    // branch inside the statement, so the compiler sees one definition of the accumulator either way.
    if constexpr (COND) {
#define AURA_SKIP_IN "s_cmp_eq_u32 %3, 0\n\ts_cbranch_scc1 .Laura_skip%=\n\t"
#define AURA_SKIP_OUT "\n.Laura_skip%=:"
#define AURA_NOP1C "s_nop 1\n\t"
#define AURA_MFMAC AURA_MFMA_OP
        if constexpr (PAD) {
            if constexpr (QA && LAST)
                asm volatile(AURA_SKIP_IN AURA_NOP1C AURA_MFMAC "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "a"(q), "s"(on) : "scc");
            else if constexpr (QA)
                asm volatile(AURA_SKIP_IN AURA_NOP1C AURA_MFMAC "%0, %1, %2, %0" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "a"(q), "s"(on) : "scc");
            else if constexpr (LAST)
                asm volatile(AURA_SKIP_IN AURA_NOP1C AURA_MFMAC "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "v"(q), "s"(on) : "scc");
            else
                asm volatile(AURA_SKIP_IN AURA_NOP1C AURA_MFMAC "%0, %1, %2, %0" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "v"(q), "s"(on) : "scc");
        } else {
            if constexpr (QA && LAST)
                asm volatile(AURA_SKIP_IN AURA_MFMAC "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "a"(q), "s"(on) : "scc");
            else if constexpr (QA)
                asm volatile(AURA_SKIP_IN AURA_MFMAC "%0, %1, %2, %0" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "a"(q), "s"(on) : "scc");
            else if constexpr (LAST)
                asm volatile(AURA_SKIP_IN AURA_MFMAC "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "v"(q), "s"(on) : "scc");
            else
                asm volatile(AURA_SKIP_IN AURA_MFMAC "%0, %1, %2, %0" AURA_SKIP_OUT : "+a"(acc) : "v"(af), "v"(q), "s"(on) : "scc");
        }
        return;
    }
    // PAD: s_nop 1 in front = the two wait states between a VALU write of an operand register and the
    // MFMA reading it (hipcc pads nothing inside inline asm).  The fp32-row kernels need it: their A
    // fragment comes out of v_cvt_pk_bf16_f32 right before.  The bf16-row kernels run without: the A
    // fragment comes from ds_read_b128 behind an s_waitcnt, the query fragments are never rewritten and
    // the accumulator set-up is several instructions away -- tools/check_mfma_hazards.py (a CPU test)
    // verifies exactly that on the generated code of every build (0.6 ns of the 8.2 ns per MFMA).
    // LAST (the tile's final k-step): 12 wait states behind the MFMA, INSIDE the statement, because
    // the compiler may read or move the accumulator right after it (it has no idea this is an MFMA).
    // AURA_CS_EXP_*: timing experiments only (tools/build_variant.sh; results are wrong with them)
#if defined(AURA_CS_EXP_NONOP)
#define AURA_NOP1 ""
#else
#define AURA_NOP1 "s_nop 1\n\t"
#endif
#ifdef AURA_CS_EXP_NOMFMA
#define AURA_MFMA "; "
#else
#define AURA_MFMA AURA_MFMA_OP
#endif
    if constexpr (PAD) {
        if constexpr (QA && LAST)
            asm volatile(AURA_NOP1 AURA_MFMA "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" : "+a"(acc) : "v"(af), "a"(q));
        else if constexpr (QA)
            asm volatile(AURA_NOP1 AURA_MFMA "%0, %1, %2, %0" : "+a"(acc) : "v"(af), "a"(q));
        else if constexpr (LAST)
            asm volatile(AURA_NOP1 AURA_MFMA "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" : "+a"(acc) : "v"(af), "v"(q));
        else
            asm volatile(AURA_NOP1 AURA_MFMA "%0, %1, %2, %0" : "+a"(acc) : "v"(af), "v"(q));
    } else {
        if constexpr (QA && LAST)
            asm volatile(AURA_MFMA "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" : "+a"(acc) : "v"(af), "a"(q));
        else if constexpr (QA)
            asm volatile(AURA_MFMA "%0, %1, %2, %0" : "+a"(acc) : "v"(af), "a"(q));
        else if constexpr (LAST)
            asm volatile(AURA_MFMA "%0, %1, %2, %0\n\ts_nop 7\n\ts_nop 4" : "+a"(acc) : "v"(af), "v"(q));
        else
            asm volatile(AURA_MFMA "%0, %1, %2, %0" : "+a"(acc) : "v"(af), "v"(q));
    }
}
#undef AURA_SKIP_IN
#undef AURA_SKIP_OUT
#undef AURA_NOP1C
#undef AURA_MFMAC
#undef AURA_NOP1
#undef AURA_MFMA
