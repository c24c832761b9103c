/*
 * svdq_amd.h -- C ABI of the MI355X (gfx950) SVDQuant W4A4 + low-rank hot path.
 *
 * This is the drop-in boundary for the two operators the reference exports from its pybind11
 * module `nunchaku._C.ops` (reference: nunchaku/csrc/pybind.cpp:108-116, nunchaku/csrc/ops.h):
 *
 *   ops.quantize_w4a4_act_fuse_lora  (csrc/ops.h:83-112 -> src/kernels/zgemm/zgemm.h:39-46)
 *   ops.gemm_w4a4                    (csrc/ops.h:10-81  -> src/kernels/zgemm/zgemm.h:8-36)
 *
 * plus the load-time re-layout of the reference's checkpoint tensors (which are stored in NVIDIA
 * mma fragment order, nunchaku/lora/flux/packer.py:187-301,362-437) into the CDNA4 operand images
 * the kernels consume.
 *
 * Operand images.  4-bit codes (weights and activations) are held as the register image of
 * v_mfma_scale_f32_32x32x64_f8f6f4 with FP6 (e2m3) operands -- a 4-bit code is exactly an FP6 value --
 * i.e. 6 bits per code: a [ROWS, K] code matrix occupies ROWS*K*3/4 bytes (ROWS % 32 == 0,
 * K % 128 == 0).  This is 1.5x the reference's ROWS*K/2 nibble buffers; the host shim
 * (nunchaku_amd/ops) allocates the opaque activation buffers accordingly.  The bit-level layout is
 * documented in nunchaku_amd/csrc/svdq_common.h and DESIGN.md.
 *
 * Rules of the boundary (mirrors the reference's behaviour):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *     NULL means "tensor absent" (the reference's `std::optional<Tensor>` / `Tensor::valid()`).
 *   - the caller owns and allocates every buffer; the library allocates nothing and keeps no
 *     pointer after a call returns (reference: ops/gemm.py:107-110, interop/torch.h:8-23).
 *   - every call is asynchronous on the hipStream_t passed as `stream` (reference launches on the
 *     current torch stream, interop/torch.cpp:84-91; no device sync, csrc/ops.h:80).
 *   - errors are returned, never abort()ed (the reference asserts: launch_impl.cuh:44-59).
 *     0 = success; non-zero = SVDQ_E_*; svdq_last_error() gives a thread-local message.
 *   - re-entrant; no global mutable state besides the thread-local error string.
 *
 * "16-bit" below means the model dtype: SVDQ_BF16 or SVDQ_FP16 (the reference picks the kernel
 * dtype from ascales.dtype(), gemm_w4a4.cu:63-65).
 */
#ifndef SVDQ_AMD_H
#define SVDQ_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVDQ_ABI_VERSION 24

/* model dtype of the 16-bit tensors */
enum { SVDQ_BF16 = 0, SVDQ_FP16 = 1 };

/* error codes */
enum {
    SVDQ_OK = 0,
    SVDQ_E_INVALID = 1,     /* bad shape / alignment / missing tensor            */
    SVDQ_E_UNSUPPORTED = 2, /* valid in the reference, not implemented here (fp4, other head sizes, ...) */
    SVDQ_E_HIP = 3          /* a HIP runtime call failed                                    */
};

/* epilogue selector of svdq_gemm_w4a4 (the reference infers it from which tensors are valid,
 * gemm_w4a4_launch_impl.cuh:282-423; the host shim does the same inference and fills `fuse`). */
enum {
    SVDQ_FUSE_NONE = 0,        /* EpilogueDefault: store out[M,N]                (launch_impl.cuh:407-420) */
    SVDQ_FUSE_SILU = 1,        /* EpilogueSilu then store                        (gemm_base.cuh:783-792)   */
    SVDQ_FUSE_GELU_QUANT = 2,  /* GELU -> [LoraDown] -> shift+smooth+u4 requant  (launch_impl.cuh:282-309) */
    SVDQ_FUSE_RMSNORM_ROPE = 3 /* QKV: RMSNorm(q,k)+RoPE then store              (launch_impl.cuh:347-405) */
};

/* lora_act formats.  The low-rank activations lora_act[M_pad, R] are an OPAQUE hand-off between the kernel that produces
 * them (the quantiser, a GELU_QUANT epilogue, the attention kernel's fused quantiser) and the GEMM that consumes them
 * (the reference's order is NVIDIA-fragment specific, lora.cuh:61-80; only the size M_pad*R*4 bytes is visible to callers).
 *   SVDQ_LORA_ACT_F32: natural [m][r] fp32; partial sums (K slices, column tiles, heads) are combined with fp32 atomics,
 *                      so the last bits depend on their arrival order -- the reference's own behaviour (lora.cuh:82-94,323).
 *   SVDQ_LORA_ACT_Q32: natural [m][r] int64 holding value * 2^32 (Q31.32 fixed point), M_pad*R*8 bytes; partial sums are
 *                      combined with 64-bit INTEGER atomics, which are associative: the result is bit-reproducible from
 *                      run to run ("deterministic mode").  Producer and consumer must agree; the buffer must be zeroed
 *                      (all-zero bytes are 0.0 in both formats).  The sums do not depend on the launch configuration
 *                      either (tile geometry, grid, stream-K): "strict".
 *   SVDQ_LORA_ACT_Q32_RUNS (ABI 22): the same buffers and the same integer atomics BETWEEN workgroups, but a GELU_QUANT
 *                      launch on 256 x 128 tiles may first sum the column tiles one workgroup walks in a row (a "row run",
 *                      svdq_gemm_last_plan variant 1) in fp32 in LDS, in a fixed order, and convert the run's sum once: no
 *                      atomics inside a tile.  Bit-reproducible from run to run and between replicas for a given (shape,
 *                      geometry, device) -- what the deterministic mode is used for -- at about half the cost of the strict
 *                      form; NOT equal to the sums of another geometry or grid.  svdq_quantize_w4a4_act_fuse_lora and
 *                      svdq_attention treat it as SVDQ_LORA_ACT_Q32 (their partial sums have no such run). */
enum { SVDQ_LORA_ACT_F32 = 0, SVDQ_LORA_ACT_Q32 = 1, SVDQ_LORA_ACT_Q32_RUNS = 2 };

/* ------------------------------------------------------------------------------------------
 * svdq_quantize_w4a4_act_fuse_lora
 * replaces kernels::quantize_w4a4_act_fuse_lora (zgemm.h:39-46, gemm_w4a4.cuh:1097-1184).
 *
 *   lora_act[M_pad, R] = x @ lora_down            (on the un-smoothed input, fp32)
 *   x_hat = round16(x / smooth);  per (row, 64-channel group): scale = amax/7,
 *   q = sat_s4(rne(x_hat / scale));  rows >= M are treated as zero.
 *
 * act and ascales are OPAQUE (operand images private to this library):
 * act M_pad*K*3/4 bytes (FP6 image), ascales (K/64)*M_pad 16-bit (scale image), lora_act M_pad*R
 * fp32 (natural [m][r], true values).
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_quantize_args {
    const void *x;         /* [M, K] 16-bit, row stride ldx elements                          */
    const void *smooth;    /* [K] 16-bit, natural order (see svdq_repack_vec); NULL = ones    */
    const void *lora_down; /* [K*R] 16-bit in svdq_repack_lowrank(down=1) order; NULL if R==0 */
    void *act;             /* out: FP6 image of the int4 codes, M_pad*K*3/4 bytes            */
    void *ascales;         /* out: (K/64)*M_pad 16-bit, 2-byte aligned (svdq_gemm_w4a4 reads it 16-byte aligned) */
    void *lora_act;        /* out: M_pad*R fp32 -- or int64, see lora_act_format -- (zeroed + accumulated inside the call); 4-byte aligned, 8-byte as int64 */
    int32_t M;             /* actual rows                                                     */
    int32_t M_pad;         /* multiple of 256, >= M                                           */
    int32_t K;             /* multiple of 128                                                 */
    int32_t R;             /* multiple of 16 (0 = no low-rank branch)                         */
    int32_t ldx;           /* row stride of x in elements (>= K, multiple of 4)               */
    int32_t dtype;         /* SVDQ_BF16 | SVDQ_FP16                                           */
    int32_t fuse_glu;      /* non-zero: x holds rows of 2K interleaved (value, gate) pairs (ldx >= 2K, a multiple of 8; x 16-byte
                              aligned) and the op quantises round16(value * round16(silu(gate))) -- the reference's
                              load_act_to_fpsum<fuse_glu> (gemm_base.cuh:606-633).  Not with ln_stats or x2.               */
    int32_t fp4;           /* must be 0 (NVFP4 is Blackwell-only)                             */
    /* Optional fused AdaLayerNormZero front end (extension; all three or none).  The quantiser then reads
     *   x' = round16(round16(round16((x - mean) * rstd) * mod_scale) + mod_shift)
     * in place of x -- the rounding points of the reference's 16-bit torch ops `norm(x) * scale[:, None] +
     * shift[:, None]` (nunchaku/models/normalization.py:85-98,155-165, transformer_flux_v2.py:233-234; nunchaku
     * checkpoints carry the +1 of the scale inside the modulation bias, scale_shift = 0) -- for the low-rank
     * projection and the codes alike. */
    const float *ln_stats; /* [M, 2] fp32 (mean, rstd) per row, e.g. from svdq_residual_gate_stats     */
    const void *mod_scale; /* [K] 16-bit                                                              */
    const void *mod_shift; /* [K] 16-bit                                                              */
    /* Grouped launch (optional, x2 != NULL): rows [split_rows, split_rows + M2) of the OUTPUT buffers come from a
     * second input x2 (row stride ldx2) quantised with a second parameter set -- the text and image stream of a joint
     * block in one launch, feeding svdq_gemm_args.wgt2.  Then M must equal split_rows (a multiple of 256). */
    const void *x2, *smooth2, *lora_down2, *mod_scale2, *mod_shift2;
    const float *ln_stats2;
    int32_t M2, ldx2, split_rows;
    int32_t lora_act_zeroed; /* non-zero: the caller guarantees lora_act is already zero on this stream (e.g. cleared by
                                svdq_residual_gate_stats' zero_ptr), so the hipMemsetAsync of the K-sliced reduction is skipped */
    int32_t lora_act_format; /* SVDQ_LORA_ACT_F32 (lora_act: M_pad*R fp32) | SVDQ_LORA_ACT_Q32 (M_pad*R int64, deterministic) */
    int32_t reserved;
} svdq_quantize_args;

/* Alignment of the operands of svdq_quantize_w4a4_act_fuse_lora ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   act                                                         16 bytes
 *   x, smooth, lora_down, ln_stats, mod_scale, mod_shift        8 bytes (x: 16 with fuse_glu)
 *   x2, smooth2, lora_down2, ln_stats2, mod_scale2, mod_shift2  8 bytes
 *   lora_act                                                    4 bytes in fp32, 8 in the Q31.32 formats
 *   ascales                                                     2 bytes
 *   ldx, ldx2                                                   4 elements (ldx: 8 with fuse_glu)
 * The fast kernel fetches lora_down(2) in 16-byte pieces by LDS-DMA, from 8-byte addresses where the caller passes one (section 7 says what was observed). */
/* Addressing reach ("Addressing reach"; refused or re-routed on the host, never wrapped on the device):
 *   ldx, ldx2           unbounded: the general kernel forms row addresses in 64 bits.  The fast kernel reads x through a buffer descriptor with 32-bit byte
 *                       offsets; a launch takes it only while M_pad * max(ldx, ldx2) * 2 < 0x7fffffff and R * K * 2 < 0x7fffffff (svdq_quantize_plan)
 *   M_pad * K, M_pad * R  unbounded: 64-bit products */
int svdq_quantize_w4a4_act_fuse_lora(const svdq_quantize_args *args, void *stream);

/* Host only, launches nothing (the quantiser's svdq_gemm_plan): validates `args` exactly as svdq_quantize_w4a4_act_fuse_lora does (same return codes and
 * messages), then writes what that launch would take -- the launch reads the same function and decides nothing else:
 *   out8[0]  kernel family: 0 = fast (quantize_kernel_v2, 32-bit byte offsets into x), 1 = general (quantize_kernel, 64-bit row addresses)
 *   out8[1]  fast: the quantize_kernel_v2 switch set (bit 0 smooth, bit 1 LayerNorm front end, bit 2 low rank, bit 3 rank > 32);
 *            general: the quantize_kernel rank class (0, 1, 2, 4, 8 tiles of 32 ranks)
 *   out8[2]  chunks of 128 columns per workgroup (cpw)      out8[3]  K slices per row tile
 *   out8[4]  lora_act_add mode: bit 0 = atomics (K is sliced), bit 1 = Q31.32 format
 *   out8[5]  grid      out8[6]  fuse_glu      out8[7]  1 = the launch clears lora_act first */
int svdq_quantize_plan(const svdq_quantize_args *args, int32_t out8[8]);

/* ------------------------------------------------------------------------------------------
 * svdq_gemm_w4a4
 * replaces kernels::gemm_w4a4 (zgemm.h:8-36, gemm_w4a4_launch_impl.cuh:7-424).
 *
 *   y[m,n] = sum_g ascales[g,m]*wscales[g,n] * (sum_{k in g} act[m,k]*wgt[n,k])      (int4 x int4)
 *            + bias[n] + sum_r round16(lora_act_in[m,r]*lora_scales[r/16]) * lora_up[n,r]
 *   then the epilogue selected by `fuse`.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_gemm_args {
    const void *act;          /* FP6 image of the activations (quantize or a GELU_QUANT gemm)  */
    const void *wgt;          /* FP6 image of the weights (svdq_repack_qweight), N*K*3/4 bytes */
    const void *ascales;      /* (K/64)*M_pad 16-bit, scale image                              */
    const void *wscales;      /* (K/64)*N 16-bit, scale image (svdq_repack_wscales)            */
    const void *bias;         /* [N] 16-bit natural order or NULL                              */
    const void *lora_act_in;  /* M_pad*R fp32 (or int64, see lora_act_format) or NULL          */
    const void *lora_up;      /* [N, R] 16-bit natural row-major (svdq_repack_lowrank(down=0)) */
    const float *lora_scales; /* HOST pointer, R/16 floats, or NULL (= all 1.0)                */
    void *out;                /* [M, N] 16-bit, row stride ldo; required unless GELU_QUANT     */
    /* SVDQ_FUSE_GELU_QUANT: this layer emits the NEXT layer's quantized activation */
    void *qout;               /* FP6 image of the uint4 codes, M_pad*N*3/4 bytes               */
    void *oscales;            /* (N/64)*M_pad 16-bit, scale image, 2-byte aligned              */
    const void *next_smooth;  /* [N] 16-bit natural order                                      */
    const void *next_lora_down; /* [N*R2] 16-bit, svdq_repack_lowrank(down=1) order, or NULL   */
    void *lora_act_out;       /* M_pad*R2 fp32 (or int64, see lora_act_format); MUST be zeroed by the caller on the
                                 same stream (reference: lora_act_out.zero_(), launch_impl.cuh:252) */
    /* SVDQ_FUSE_RMSNORM_ROPE */
    const void *norm_q;       /* [128] 16-bit                                                   */
    const void *norm_k;       /* [128] 16-bit                                                   */
    const float *rotary_emb;  /* [M_pad, 128] fp32 in the reference's pack_rotemb order
                                 (models/embeddings.py:100-138)                                 */
    int32_t M;                /* actual rows (rows >= M are not stored to `out`)                */
    int32_t M_pad;            /* multiple of 256                                                */
    int32_t N;                /* multiple of 128                                                */
    int32_t K;                /* multiple of 128                                                */
    int32_t R;                /* rank of lora_up (multiple of 16 in [0, 256]; 0 = none).  Every rank runs the fused path; 32 (the SVDQuant default),
                               * 48 .. 160 (the r128 checkpoints, a runtime LoRA on top of rank 32) have kernels of their own */
    int32_t R2;               /* rank of next_lora_down (multiple of 16 in [0, 256]; 0 = none)  */
    int32_t ldo;              /* row stride of out in elements (>= N)                           */
    int32_t dtype;            /* SVDQ_BF16 | SVDQ_FP16                                          */
    int32_t act_unsigned;     /* informational: the FP6 image already encodes signedness        */
    int32_t fuse;             /* SVDQ_FUSE_*                                                    */
    int32_t variant;          /* must be 0 */
    int32_t reserved;         /* must be 0 */
    /* optional scratch for the stream-K tail (svdq_gemm_workspace_bytes() bytes, zero-filled ONCE by the
     * caller, then reusable by every later call ON THE SAME STREAM; NULL = whole-tile schedule only).
     * One workspace must never be used by launches that can be in flight concurrently (two streams, two
     * threads on different streams): keep one per (device, stream), as nunchaku_amd/_C.py does.  A violated
     * contract cannot hang the GPU -- an owner's wait is bounded -- but it invalidates the results; it is
     * reported by svdq_gemm_workspace_status().
     * Only the header -- the first 8192 bytes: arrival counters, error word, ticket counters -- needs the one-time zero fill, and every
     * launch leaves all of it at zero.  The bytes behind it (partial-tile slabs, packed low-rank images, the split's 16-bit image) need no
     * initialisation: a launch reads none it did not write itself, so they may hold anything, NaN patterns and the leftovers of a launch
     * of another shape, geometry or epilogue included (tests/test_gpu_workspace_hygiene.py). */
    void *workspace;
    int64_t workspace_bytes;
    /* SVDQ_FUSE_RMSNORM_ROPE only, optional: the V third of the output (columns [2N/3, N)) is written
     * TRANSPOSED, element (m, n) -> out_vt[(n - 2N/3) * ldvt + m], and NOT to `out` -- the key-contiguous
     * operand svdq_attention reads (role of the reference's packed out_v, epilogues.cuh:427-550).  A joint
     * (text + image) attention passes the same buffer to both GEMMs with out_vt offset by the token start. */
    void *out_vt;
    int32_t ldvt;             /* row stride of out_vt in elements (>= total tokens)              */
    /* Workgroup geometry: 0 = chosen by the library; 1 = 256 x 128 tiles, one 512-thread workgroup per CU, fixed tile list
     * per workgroup + stream-K tail; 2 = 128 x 128 tiles, two 256-thread workgroups per CU (one's epilogue and barrier
     * stalls under the other's main loop) that DRAW their tiles from per-XCD queues in the workspace (falls back to 3 without
     * a workspace, for launches of at most one tile per workgroup, and where a stream-K split pays); 3 = 128 x 128 tiles,
     * fixed tile lists + stream-K tail; 4 / 5 = 2 / 3 with the second workgroup of a CU started half a tile late (A/B
     * measurements); 6 = GELU_QUANT launches with a next-layer low-rank branch of rank <= 128 (fp32 accumulators) run 128 x 128 tiles with ONE
     * workgroup per CU, whose LDS then holds the low-rank-down carry of a whole run of column tiles (what geometry 0 picks for next-layer ranks
     * 48 .. 128 at two or more tiles per CU; 6 asks for it at any size -- tests), every other launch as with 0; 7 (ABI 20) = GELU_QUANT launches with a
     * next-layer low-rank branch of rank 48 .. 160 run it SPLIT (256 x 128 tiles whose epilogue stores the 16-bit GELU output as MFMA fragments into the
     * workspace, a second kernel contracts them with next_lora_down; needs a workspace of svdq_gemm_workspace_bytes_for() bytes and R in 48 .. 160; what
     * geometry 0 picks for those ranks from a full round of tiles; 7 asks for it at any size), every other launch as with 0;
     * 8 (ABI 21) = the plain epilogue at rank 0 / 32 (fp32 low-rank accumulators) runs the 128 x 64-per-wave kernel (plan variant 6), every other launch as with 0.
     * Results are bit-identical across geometries for launches without a stream-K split (the split points, hence the fp32 summation order of a split tile, differ); lora_act_out
     * differs by fp32 summation order between all of them (atomics). */
    int32_t geometry;
    /* Grouped launch (optional): rows [split_rows, M_pad) use a SECOND weight set of the same shape, rank and
     * epilogue -- one launch for the text and the image stream of a joint FLUX block (same layer type, different
     * weights, transformer_flux_v2.py:200-260), whose row-side tensors (act, ascales, lora_act_in, out, qout,
     * oscales, lora_act_out, rotary_emb, out_vt) are simply the two streams' buffers back to back.  The 48..192
     * tiles of the 512-token stream then fill the tail of the big GEMM's last round instead of running as a
     * launch-latency-bound GEMM of their own.  wgt2 == NULL: off.  bias / bias2 must both be given or both NULL. */
    const void *wgt2, *wscales2, *bias2, *lora_up2;
    const void *next_smooth2, *next_lora_down2; /* GELU_QUANT */
    const void *norm_q2, *norm_k2;              /* RMSNORM_ROPE */
    int32_t split_rows;       /* multiple of 256, 0 < split_rows < M_pad                         */
    int32_t lora_act_format;  /* SVDQ_LORA_ACT_F32 | SVDQ_LORA_ACT_Q32: format of lora_act_in AND lora_act_out */
    /* Optional host-visible status word (pinned, device-accessible host memory: hipHostMalloc / a torch pinned tensor), or
     * NULL.  A stream-K owner that gives up waiting for partial tiles (see `workspace`) stores 1 here with system scope:
     * the host can poll it WITHOUT synchronising -- nunchaku_amd/_C.py checks it before every launch on the same stream
     * and raises.  The co-residency the persistent schedule relies on: the whole grid (<= 1 or 2 workgroups per CU,
     * depending on the geometry) must become resident while owners wait -- true for a stream that owns the device, not for
     * a CU-masked stream or beside a long-running co-tenant kernel; pass workspace = NULL there. */
    int32_t *status;
    /* SVDQ_FUSE_RMSNORM_ROPE only (extension): the Q third (columns [0, N/3)) is multiplied by q_scale inside the epilogue, BEFORE
     * its single rounding to 16-bit (0 = off = 1.0; q_scale = 1.0 is bit-identical to off).  For svdq_attention_args.q_prescaled: the
     * attention kernel then needs no per-score scaling, and Q carries one rounding as in the reference (scaling an already rounded Q
     * inside the attention kernel would add a second one). */
    float q_scale;
    int32_t reserved2;        /* must be 0 */
    /* ABI 21, optional (NULL = the launch packs them itself, as ABI 19 / 20 did on every launch): the weight-side operands of the rank 48 .. 160 kernels as MFMA
     * fragments, packed ONCE per parameter with svdq_pack_lora_down / svdq_pack_lora_up (nunchaku_amd/_C.py caches them per storage and version, so a set_lora
     * re-packs).  next_lora_down_packed(2): used by a launch whose next-layer low-rank down projection runs split (plan variant 5); lora_up_packed: by the
     * kernels that read lora_up as fragments (128 x 128 tiles at rank 48 .. 160, the solo-carry kernel).  Must hold the image of the very tensor passed in
     * next_lora_down(2) / lora_up. */
    const void *next_lora_down_packed, *next_lora_down_packed2;
    const void *lora_up_packed;
} svdq_gemm_args;

/* Alignment of the operands of svdq_gemm_w4a4 ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   act, wgt, ascales, wscales, lora_act_in, lora_up, qout, rotary_emb, workspace            16 bytes
 *   wgt2, wscales2, lora_up2, lora_up_packed, next_lora_down_packed, next_lora_down_packed2  16 bytes
 *   out, bias, next_smooth, next_lora_down, lora_act_out, norm_q, norm_k                     8 bytes
 *   bias2, next_smooth2, next_lora_down2, norm_q2, norm_k2                                   8 bytes
 *   out_vt, status                                                                           4 bytes
 *   oscales                                                                                  2 bytes
 *   ldo                                                                                      4 elements: every row of out starts on 8 bytes
 *   ldvt                                                                                     2 elements: every row of out_vt starts on 4 bytes
 * lora_scales is a HOST pointer to floats.  out is stored in 16-byte pieces, at 8-byte addresses where out or ldo put a row there (section 7). */
/* Addressing reach ("Addressing reach"):
 *   ldo                 unbounded.  The wave-tile kernel's epilogue stores take a 32-bit byte offset (254 * ldo + 16 over a wave's 128 rows): it serves
 *                       ldo <= 16909316; a launch with a wider out takes the 8-wave kernel (64-bit row addresses); svdq_gemm_plan answers which
 *   ldvt                at most 429496716: the QKV epilogue's lane offset 10 * ldvt + 124 is a 32-bit byte offset; beyond: SVDQ_E_UNSUPPORTED
 *   M_pad * N, M_pad * K  unbounded: 64-bit products */
int svdq_gemm_w4a4(const svdq_gemm_args *args, void *stream);

/* ABI 21: the fragment images above.  ld = [R2][N] rank-major (svdq_repack_lowrank(down=1) order), R2 in 48 .. 160, N % 256 == 0 (or R2 = 16 / 32, N % 128 == 0: the
 * one-block image the attention epilogue's quantiser reads, svdq_attention_args.qlora_down_packed) -> out, svdq_pack_lora_down_bytes(N, R2)
 * bytes ([N / 16 units][ceil(R2 / 32) rank blocks][64 lanes][8] 16-bit, ranks >= R2 zero); lu = [N][R] natural -> out, svdq_pack_lora_up_bytes(N, R) bytes
 * ([N / 32][R / 16][64 lanes][8]).  Pure permutations (a weight changes only under a set_lora): pack once, pass with every launch. */
int64_t svdq_pack_lora_down_bytes(int32_t N, int32_t R2);
int svdq_pack_lora_down(const void *ld, void *out, int32_t N, int32_t R2, int32_t dtype, void *stream);
int64_t svdq_pack_lora_up_bytes(int32_t N, int32_t R);
int svdq_pack_lora_up(const void *lu, void *out, int32_t N, int32_t R, int32_t dtype, void *stream);
/* size of the GEMM workspace for the current device: 1023 arrival counters + 1 error word + 2 fp32 tiles of 256 x 128 per CU (the stream-K tail), and
 * -- ABI 19 -- a 24 MB tail in which a launch of rank 48 .. 160 keeps its low-rank operands as packed 16-bit MFMA fragments (written by a small pack
 * kernel the call enqueues in front of the GEMM; valid, like the rest, for launches ordered on ONE stream).  Without a workspace (or with one of the
 * ABI 18 size) such launches take the plain kernels' rank > 32 path: same results, a memory round trip per 16 ranks in every tile's epilogue. */
int64_t svdq_gemm_workspace_bytes(void);
/* ABI 20: the workspace size with which THIS launch takes every fast path it has: svdq_gemm_workspace_bytes(), plus M_pad * N * 2 bytes for a GELU_QUANT
 * launch whose next-layer low-rank down projection can run split (geometry 7 above; geometry 0 for next-layer ranks 48 .. 160 from a full round of tiles).  Only shapes, ranks, fuse, geometry,
 * lora_act_format and the operand pointers' alignment are read.  A workspace of svdq_gemm_workspace_bytes() bytes is never an error: such a launch then runs
 * the solo-carry / hybrid-carry kernels. */
int64_t svdq_gemm_workspace_bytes_for(const svdq_gemm_args *args);
/* What the calling thread's last svdq_gemm_w4a4 launched (ABI 19; a test / diagnostics aid, no effect on results): out8 = {tile rows (256 | 128), kernel variant,
 * grid, stream-K groups (0 = whole tiles), row-run length (0 = plain schedule), lora_act_in packed (0 | 1), lora_up packed (0 | 1), dynamic tile queue (0 | 1)}.
 * Variants: 0 plain (rank <= 32 staged / any rank through the fallback loads; GELU_QUANT: per-tile atomics), 1 low-rank-down carry (GELU_QUANT, next rank <= 32),
 * 2 all-rank (rank 48 .. 160: packed lora_act_in; 256-row tiles: lora_up staged in LDS, 128-row tiles: lora_up packed too), 3 hybrid carry (GELU_QUANT, next rank
 * 48 .. 80 -- or any next rank > 32 the solo kernel does not take; behind variant 5), 4 solo carry (GELU_QUANT, next rank >= 96: 128 x 128 tiles, one workgroup per CU; behind variant 5),
 * 5 split low-rank down (ABI 20: GELU_QUANT, next rank 48 .. 160 with a workspace of svdq_gemm_workspace_bytes_for() bytes: all-rank kernel on 256-row tiles
 * + lowrank_down_split_kernel), 6 wave tile 128 (ABI 21: the plain epilogue at rank 0 / 32 on 256 x 128 tiles with FOUR waves of 128 x 64 each, one per SIMD --
 * generated loop AND epilogue, bit-identical to variant 0; geometry 8 asks for it, geometry 0 picks it wherever it would have launched 256-row tiles). */
#define SVDQ_PLAN_PLAIN 0
#define SVDQ_PLAN_CARRY 1
#define SVDQ_PLAN_ALL_RANK 2
#define SVDQ_PLAN_HYBRID_CARRY 3
#define SVDQ_PLAN_SOLO_CARRY 4
#define SVDQ_PLAN_SPLIT_DOWN 5
#define SVDQ_PLAN_WAVE_TILE_128 6
int svdq_gemm_last_plan(int32_t *out8);
/* Host only, launches nothing (the GEMM's svdq_attention_plan): validates `args` exactly as svdq_gemm_w4a4 does (same return codes and messages), then writes the
 * eight words svdq_gemm_last_plan would report after that launch on a device of `cus` compute units (1 .. 256; 0 = the current device's count, 256 where there
 * is none).  Reads the shapes, ranks, fuse, geometry, lora_act_format, workspace_bytes and which pointers are NULL / 16-byte aligned; dereferences none of them.
 * Launch and query run the same function (plan_gemm, csrc/gemm_w4a4.hip), so a test can pin the dispatch without a GPU (tests/test_gemm_plan.py).  One new
 * symbol, nothing existing changes, so SVDQ_ABI_VERSION stays 24. */
int svdq_gemm_plan(const svdq_gemm_args *args, int32_t cus, int32_t out8[8]);
/* Synchronises `stream`, then returns SVDQ_E_HIP (and clears the flag) if a launch that used `workspace` timed out
 * waiting for partial tiles -- see svdq_gemm_args.workspace; SVDQ_OK otherwise.  Test / debugging aid. */
int svdq_gemm_workspace_status(void *workspace, void *stream);
/* Host-side replay of the kernel's persistent / stream-K schedule (test helper; no GPU needed): writes up to
 * `cap` records of 6 int32 {position, tile, kp0, kp1, partial slot or -1, contributors the owner waits for}
 * and returns the number of segments, or -1 for invalid shapes. */
int svdq_gemm_schedule(int32_t M_pad, int32_t N, int32_t K, int32_t cus, int32_t with_workspace, int32_t *out, int32_t cap);
/* the same for an explicit geometry (1 or 2, see svdq_gemm_args.geometry); svdq_gemm_schedule is geometry 1.
 * geometry 3 replays the ROW-RUN schedule a GELU_QUANT launch of geometry 1 takes when it has a next-layer low-rank branch of rank <= 32, no K
 * split and at least two tiles per workgroup (every workgroup walks one run of consecutive column tiles of one row block, so that the next
 * layer's low-rank down projection is accumulated inside the workgroup and written once per run): tile ids are row-major there
 * (tile = row_block * (N / 128) + column_tile); -1 when such a launch would take the plain schedule. */
int svdq_gemm_schedule_ex(int32_t M_pad, int32_t N, int32_t K, int32_t cus, int32_t with_workspace, int32_t geometry,
                          int32_t *out, int32_t cap);

/* ------------------------------------------------------------------------------------------
 * Attention over the packed QKV (reference: ops.attention_fp16, nunchaku/csrc/ops.h:114-121,
 * src/kernels/zgemm/attention.cu:11-94).  Non-causal, optional key-padding mask,
 * head_dim 128, one batch element per call:
 *   O[l, h, :] = softmax_j(scale * Q[l, h, :] . K[j, h, :]) V[j, h, :]
 * element addresses (in 16-bit elements):
 *   Q (l,h,d): q  + l*ldq  + h*q_hs  + d        K (j,h,d): k + j*ldk + h*k_hs + d
 *   V (j,h,d): vt + d*ldvt + h*vt_hs + j        (V TRANSPOSED: keys contiguous)
 *   O (l,h,d): out + l*ldo + h*o_hs  + d
 * With the fused QKV GEMM output [L, 3*H*128] (+ out_vt [H*128, L]): q = qkv, k = qkv + H*128,
 * ldq = ldk = 3*H*128, q_hs = k_hs = 128, vt_hs = 128*ldvt, out [L, H*128]: o_hs = 128, ldo = H*128.
 * L (queries = keys) must be a multiple of 128 (the models pad tokens to 256: fused.py:140-152).
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_attention_args {
    const void *q, *k, *vt;
    void *out;
    int64_t q_hs, k_hs, vt_hs, o_hs; /* head strides in elements */
    int32_t ldq, ldk, ldvt, ldo;     /* token (q, k, out) / channel (vt) strides in elements */
    int32_t L, H, head_dim, dtype;
    float scale;                     /* softmax scale, e.g. 1/sqrt(head_dim) */
    int32_t reserved;
    /* optional: zero-fill an unrelated scratch buffer in the same launch (the fp32 low-rank accumulators of the output
     * projection's quantiser, see svdq_residual_args.zero_ptr).  zero_bytes must be a multiple of 16. */
    void *zero_ptr;
    int64_t zero_bytes;
    /* Optional fused quantiser (extension): the output projection that follows reads the attention output only through
     * svdq_quantize_w4a4_act_fuse_lora, and a wave's 32 query rows x 128 channels of one head ARE one F6 chunk in the
     * register layout it already holds -- so the kernel can emit that projection's quantised activation directly
     * (same arithmetic as the quantiser on the 16-bit rounded output: bit-identical codes and scales; lora_act summed
     * over the H heads with fp32 atomics).  qact != NULL enables it; out may then be NULL.  Requires L % 256 == 0,
     * K = H*128, R a multiple of 16 <= 256 (32 ranks per pass; rank 48 .. 160 with a workspace of svdq_attention_workspace_bytes_for()
     * bytes: a contraction kernel behind the attention kernel, ABI 20), and qlora_act zeroed by the caller on this stream.
     * Rows >= qsplit_rows (a multiple of 256; 0 = off) use qsmooth2 / qlora_down2 (joint attention: text rows first). */
    void *qact;               /* FP6 image, L * (H*128) * 3/4 bytes                                 */
    void *qscales;            /* scale image, (H*128/64) * L 16-bit, 2-byte aligned                 */
    void *qlora_act;          /* [L, R] fp32 (or int64: qlora_act_format), pre-zeroed; 4-byte aligned, 8-byte as int64 */
    const void *qsmooth, *qlora_down;   /* [H*128] natural; [R][H*128] rank-major (svdq_repack_lowrank(down=1)) */
    const void *qsmooth2, *qlora_down2;
    int32_t qR, qsplit_rows;
    /* optional scratch of the persistent schedule (svdq_attention_workspace_bytes() bytes, zero-filled ONCE by the caller;
     * the kernel leaves its counters at zero).  A task = (head, 256 query rows) x all KV tiles; when the tasks do not fill
     * whole rounds of compute units (FLUX.1 at 1024^2: 432 tasks on 256 CUs) the launch becomes one workgroup per CU, the
     * KV tiles of all tasks dealt evenly, partial (O, m, l) exchanged through this buffer.  Same contract as
     * svdq_gemm_args.workspace: never shared by launches that can be in flight concurrently; a waiting workgroup gives up
     * after ~1 s and raises the error word svdq_attention_workspace_status() reports.  NULL (or too small): plain grid.
     * Results of the two schedules differ by fp32 summation order only.
     * Only the header -- the first 4096 bytes: arrival counters and the error word -- needs the one-time zero fill, and every launch leaves
     * all of it at zero.  The bytes behind it (contributor and stash slabs, the split quantiser's packed factor and row image) need no
     * initialisation: a launch reads none it did not write itself (tests/test_gpu_workspace_hygiene.py). */
    void *workspace;
    int64_t workspace_bytes;
    int32_t qlora_act_format; /* SVDQ_LORA_ACT_F32 | SVDQ_LORA_ACT_Q32 (deterministic head sum) */
    int32_t q_prescaled;      /* non-zero: Q already carries the factor scale * log2(e) (svdq_gemm_args.q_scale of the QKV GEMM that wrote
                                 it); `scale` is then not applied again.  Either geometry. */
    int32_t *status;          /* optional host-visible status word, as svdq_gemm_args.status */
    /* Key-padding mask (optional; kv_len0 == 0: every one of the L keys is real).  Keys [0, kv_len0) and [kv_start1, kv_end1) are
     * real tokens, all others are padding and get probability 0 -- the token buffers of a pipeline are padded to a multiple of
     * 128 / 256 rows (L itself stays a multiple of 128), a joint [text | image] sequence padded per stream has its padding in the
     * middle: hence two ranges (kv_start1 = kv_end1 = 0: one range).  Padded K / Q rows may hold anything, including NaN; padded
     * V^T columns must be FINITE (0 * NaN is NaN in the matrix unit): zero them.  Output rows of padded queries are unspecified.
     * Role of the reference's padded-row masking (epilogues.cuh:427-550, attention.cuh). */
    int32_t kv_len0, kv_start1, kv_end1;
    /* workgroup geometry: 0 = automatic; 1 = 8 waves x 32 query rows (two waves per SIMD); 2 = 4 waves x 64 query rows (one wave per
     * SIMD with the whole register file, the tile loop in generated assembly; needs L % 256 == 0 and no key mask -- masked launches run
     * geometry 1).  Geometry 2 keeps its scores relative and in log2 units, which needs Q multiplied by scale * log2(e): with q_prescaled
     * the producer has done that (one rounding, as accurate as geometry 1); otherwise the kernel scales the 16-bit Q itself -- a second
     * rounding, ~2.5x the error of geometry 1 against an fp32 reference.  Hence automatic = geometry 2 (on the plain grid) iff
     * q_prescaled, L % 256 == 0 and no mask; an explicit geometry uses the persistent schedule when a workspace is given. */
    int32_t geometry;
    /* ABI 21, optional: qlora_down(2) as the fragment image of svdq_pack_lora_down (N = H * 128) for a launch whose fused quantiser runs its low-rank down
     * projection split (rank 48 .. 160 with the workspace of svdq_attention_workspace_bytes_for()); NULL = packed by the launch.
     * Also read at qR = 16 / 32 (an addition within ABI 24: until now the fields were ignored at these ranks, and svdq_pack_lora_down refused them, so no
     * existing caller can have set them): the same image at one rank block (svdq_pack_lora_down(N = H * 128, R2 = qR); ranks >= qR zero), 16-byte aligned.  The
     * epilogue's low-rank pass then requests the head's factor once per task as lane-contiguous 16-byte loads instead of row-per-lane 8-byte loads per row
     * tile; same results bit for bit.  A launch with two weight sets (qsmooth2) takes this path only when BOTH images are given; NULL = the rank-major rows. */
    const void *qlora_down_packed, *qlora_down_packed2;
} svdq_attention_args;

/* Alignment of the operands of svdq_attention ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   q, k, vt, out, zero_ptr, qact, workspace, qlora_down_packed, qlora_down_packed2  16 bytes
 *   qsmooth, qlora_down, qsmooth2, qlora_down2                                       8 bytes
 *   qlora_act                                                                        4 bytes in fp32, 8 in the Q31.32 formats
 *   status                                                                           4 bytes
 *   qscales                                                                          2 bytes
 *   ldq, ldk, ldvt, ldo, q_hs, k_hs, vt_hs, o_hs                                     8 elements */
/* Addressing reach ("Addressing reach"):
 *   ldk                 at most 33554424: the geometry-2 loop keeps the K tile stride 128 * ldk in a 32-bit scalar (and key row 63 of a tile sits at the
 *                       32-bit byte offset 126 * ldk + 240); beyond: SVDQ_E_UNSUPPORTED
 *   ldvt                at most 16909312: channel row 127 of a V^T tile sits at the 32-bit byte offset 254 * ldvt + 112; beyond: SVDQ_E_UNSUPPORTED
 *   ldq, ldo, q_hs, k_hs, vt_hs, o_hs   unbounded: 64-bit row and head addresses */
int svdq_attention(const svdq_attention_args *args, void *stream);
/* size of the persistent-schedule workspace for the current device (1023 arrival counters + 1 error word + two fp32 slabs per CU: the part a
 * contributor publishes and, for geometry 2, the part the owner of a split task parks while it runs its whole tasks) */
int64_t svdq_attention_workspace_bytes(void);
/* ABI 20: the workspace size with which THIS launch takes every fast path it has: svdq_attention_workspace_bytes(), plus -- fused quantiser (qact) with fp32
 * accumulators, rank 48 .. 160 and H * 128 a multiple of 256 -- the room its low-rank down projection needs to run SPLIT: the kernel's epilogue stores the
 * normalised 16-bit rows as MFMA operand fragments (L * H * 128 * 2 bytes) instead of contracting them in 2 .. 5 passes of atomics that all H heads aim at the same
 * elements, and a streaming kernel behind it contracts that image with qlora_down (the kernel svdq_gemm_w4a4 uses for a GELU_QUANT launch's next layer; packed
 * copies of qlora_down / qlora_down2 sit in front of the image).  Only shapes, ranks, formats and which pointers are given are read.  A workspace of
 * svdq_attention_workspace_bytes() bytes is never an error: the kernel then runs its in-epilogue passes.  qlora_act differs by fp32 summation order. */
int64_t svdq_attention_workspace_bytes_for(const svdq_attention_args *args);
/* Synchronises `stream`, then returns SVDQ_E_HIP (and clears the flag) if a launch that used `workspace` timed out waiting
 * for partial results; SVDQ_OK otherwise.  Test / debugging aid. */
int svdq_attention_workspace_status(void *workspace, void *stream);
/* Host-side replay of the persistent schedule for (L, H) on `cus` compute units: up to `cap` records of 6 int32
 * {workgroup, task = head * (L/256) + query tile, first KV tile, end KV tile, owner workgroup or -1 (this segment owns its
 * task), last contributing workgroup or -1 (no other contributor)}; returns the number of segments, 0 when the problem runs
 * on the plain grid (L % 256 != 0 or whole rounds of tasks), -1 on bad arguments.  No GPU needed. */
int svdq_attention_schedule(int32_t L, int32_t H, int32_t cus, int32_t *out, int32_t cap);
/* Which kernel a launch with these arguments would take (host only; pointers are not looked at): out[0] = workgroup geometry (1 / 2), out[1] = 1 when
 * the key mask runs on geometry 2 (round 4: q_prescaled or an explicit geometry 2, L % 256 == 0, a run of at least two fully real 64-key tiles),
 * out[2], out[3] = the main segment [j0, j1) of fully real tiles its assembly loop walks -- the remaining tiles that hold a real key run as C++ "extra"
 * tiles that continue the softmax state, tiles without a real key are skipped. */
int svdq_attention_plan(const svdq_attention_args *args, int32_t out[4]);
/* What the calling thread's last svdq_attention launched (ABI 20; a test / diagnostics aid): out4 = {workgroup geometry (1 | 2), workgroups of the persistent
 * schedule (0 = plain grid), key mask on geometry 2 (0 | 1), the fused quantiser's low-rank down projection ran split (0 | 1)}. */
int svdq_attention_last_plan(int32_t *out4);

/* ------------------------------------------------------------------------------------------
 * Gated residual + LayerNorm statistics (extension; the element-wise glue between the operators of a block,
 * transformer_flux_v2.py:118-342):
 *   t = b ? round16(a + b) : a;      if (gate) t = round16(gate[c] * t);      y = a ? round16(res + t) : res;   [fp16: optional clip]
 *   out[m, :] = y (if out);          stats[m] = (mean(y), 1/sqrt(var(y) + eps)) over the 16-bit values (if stats)
 * i.e. the reference's 16-bit torch ops `residual + gate.unsqueeze(1) * (attn [+ mlp])`
 * (transformer_flux_v2.py:230-251,332-335) with the statistics the next LayerNorm needs produced in the same pass.  out may alias res.  C must be a multiple of 8 with ceil(C/512) in {1..8, 12, 16, 24, 32}.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_residual_args {
    const void *res;   /* [M, C] 16-bit, row stride ld */
    const void *a;     /* [M, C] or NULL (statistics of res only) */
    const void *b;     /* [M, C] or NULL */
    const void *gate;  /* [C] 16-bit or NULL */
    void *out;         /* [M, C] or NULL */
    float *stats;      /* [M, 2] fp32 or NULL */
    int32_t M, C, ld;  /* ld: common row stride of res / a / b / out in elements */
    int32_t dtype;
    float eps;
    int32_t clamp_fp16; /* SVDQ_FP16 only: bit 0 (first problem) / bit 1 (second problem) set: y is clipped to +-65504 before
                           the store and the statistics -- the reference's fp16 blocks clip the text stream after a joint
                           block and the hidden state after a single block (transformer_flux_v2.py:254-255, 339-340) */
    /* optional: zero-fill an unrelated scratch buffer in the same pass (the fp32 low-rank accumulators of the
     * quantiser / GELU_QUANT calls that follow: saves their memset launches).  zero_bytes must be a multiple of 16. */
    void *zero_ptr;
    int64_t zero_bytes;
    /* Grouped launch (optional, res2 != NULL): a second, independent problem of the same width C and row stride
     * (M2 rows; the text stream of a joint block beside the image stream) in the same launch.  a2 / b2 / gate2 /
     * out2 / stats2 must mirror a / b / gate / out / stats in being given or NULL. */
    const void *res2, *a2, *b2, *gate2;
    void *out2;
    float *stats2;
    int32_t M2;
    int32_t reserved2;
} svdq_residual_args;

/* Alignment of the operands of svdq_residual_gate_stats ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   res, a, b, gate, out, zero_ptr, res2, a2, b2, gate2, out2  16 bytes
 *   stats, stats2                                              8 bytes
 *   ld                                                         8 elements */
/* Addressing reach ("Addressing reach"):
 *   ld                  the field's width: (size_t)row * ld
 *   M, M2, M * ld       int32 row counts; the product is 64-bit
 *   zero_bytes          int64 */
int svdq_residual_gate_stats(const svdq_residual_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Residual difference (ABI 24; the decision pass of First-Block Cache.  reference: nunchaku/caching/utils_v2.py:133,176
 * `hidden - original`, fbcache.py:275-277 `(t1 - t2).abs().mean() / t1.abs().mean()`, 16-bit torch ops):
 *   r[m, c] = base ? round16(cur[m, c] - base[m, c]) : cur[m, c];        out_res[m, c] = r[m, c]   (if out_res)
 *   sum_diff = sum |round16(prev[m, c] - r[m, c])|;   sum_prev = sum |prev[m, c]|                   (if prev)
 * over rows [0, M) of [M, C] 16-bit tensors with the common row stride ld.  base == NULL compares an existing residual
 * (out_res must be NULL then); prev == NULL is the subtraction alone.  out_res may alias cur or base.
 * The sums are fp32 and bit-identical from launch to launch (no floating-point atomics): per-row sums go to `partials`, a second
 * kernel behind the first on the same stream adds them in a fixed order and fills `result`.  A term passes through at most
 * 8 * ceil(C / 512) + 6 + ceil(rows / 256) + 8 additions (rows = M + M2).  C as for svdq_residual_gate_stats.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_residual_diff_result {
    float sum_diff, sum_prev;   /* fp32 sums over both problems */
    float mean_diff, mean_prev; /* round16(sum * (1 / (rows * C))): torch's 16-bit mean, widened to fp32 */
    float ratio;                /* round16(mean_diff / mean_prev): the 16-bit quotient the reference compares with its threshold */
    int32_t rows;               /* M + M2 */
    int32_t reserved[2];
} svdq_residual_diff_result;

typedef struct svdq_residual_diff_args {
    const void *cur;   /* [M, C] 16-bit, row stride ld */
    const void *base;  /* [M, C] or NULL (r = cur) */
    const void *prev;  /* [M, C] or NULL (no sums) */
    void *out_res;     /* [M, C] or NULL */
    /* Grouped launch (optional, cur2 != NULL): a second problem of the same width and row stride (M2 rows) whose terms go
     * into the SAME two sums -- the real text rows and the real image rows of a joint sequence [text | pad | image | pad].
     * base2 / prev2 / out_res2 must mirror base / prev / out_res in being given or NULL. */
    const void *cur2, *base2, *prev2;
    void *out_res2;
    float *partials;                   /* [M + M2, 2] fp32 scratch; required with prev */
    svdq_residual_diff_result *result; /* DEVICE record; required with prev */
    int32_t M, M2, C, ld;
    int32_t dtype;
    int32_t reserved;
} svdq_residual_diff_args;

/* Alignment of the operands of svdq_residual_diff ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   cur, base, prev, out_res, cur2, base2, prev2, out_res2  16 bytes
 *   partials, result                                        8 bytes
 *   ld                                                      8 elements */
/* Addressing reach:
 *   ld                  the field's width: (size_t)row * ld
 *   M, M2, M * ld       int32 row counts (2 * (M + M2) partial sums); the product is 64-bit */
int svdq_residual_diff(const svdq_residual_diff_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Modulated-input difference (the decision pass of TeaCache; added WITHOUT a version bump: one new symbol, nothing existing changes, so
 * SVDQ_ABI_VERSION stays 24.  reference: nunchaku/caching/teacache.py:187,199-200 -- block 0's AdaLayerNormZero output and
 * `(m - prev).abs().mean() / prev.abs().mean()`, 16-bit torch ops):
 *   m[r, c] = round16( round16( round16((x[r, c] - mean[r]) * rstd[r]) * mod_scale[c] ) + mod_shift[c] )
 *   out_mod[r, c] = m[r, c]                                                                       (if out_mod)
 *   sum_diff = sum |round16(prev[r, c] - m[r, c])|;   sum_prev = sum |prev[r, c]|                  (if prev)
 * over rows [0, M) of [M, C] 16-bit tensors with the common row stride ld; rows at or beyond M are neither read nor written.
 * m has the rounding points of the quantiser's fused front end (svdq_quantize_args.ln_stats / mod_scale / mod_shift): (x - mean) in
 * fp32, and the checkpoint's scale already contains the +1.  stats is what svdq_residual_gate_stats writes.  prev and out_mod may be the
 * same buffer (the caller keeps one across steps).  prev == NULL modulates and stores only (the first step of a run); out_mod == NULL
 * with prev compares only.  The sums follow svdq_residual_diff's contract -- per-row fp32 sums to `partials`, the same finishing kernel
 * behind the first on the same stream, the same record, no floating-point atomics, bit-identical from launch to launch -- and a term
 * passes through at most 8 * ceil(C / 512) + 6 + ceil(M / 256) + 8 additions.  C as for svdq_residual_gate_stats.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_modulated_diff_args {
    const void *x;         /* [M, C] 16-bit, row stride ld */
    const float *stats;    /* [M, 2] fp32 (mean, rstd) of the rows of x; required */
    const void *mod_scale; /* [C] 16-bit */
    const void *mod_shift; /* [C] 16-bit */
    const void *prev;      /* [M, C] or NULL (no sums) */
    void *out_mod;         /* [M, C] or NULL; may alias prev */
    float *partials;                   /* [M, 2] fp32 scratch; required with prev */
    svdq_residual_diff_result *result; /* DEVICE record; required with prev */
    int32_t M, C, ld;
    int32_t dtype;
} svdq_modulated_diff_args;

/* Alignment of the operands of svdq_modulated_diff ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   x, mod_scale, mod_shift, prev, out_mod  16 bytes
 *   stats, partials, result                 8 bytes
 *   ld                                      8 elements */
/* Addressing reach:
 *   ld                  the field's width: (size_t)row * ld
 *   M, M2, M * ld       int32 row counts (2 * (M + M2) partial sums); the product is 64-bit */
int svdq_modulated_diff(const svdq_modulated_diff_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Image-prompt cross-attention (IP-Adapter; added WITHOUT a version bump: one new symbol, nothing existing changes, so
 * SVDQ_ABI_VERSION stays 24.  reference: nunchaku/models/ip_adapter/utils.py:346-372 -- a contiguous copy of Q, three
 * view-transposes, SDPA, a transpose-reshape copy and the multiply of the scaled add, torch ops there):
 *   out[t, h, :] = round16( out_scale * round16( softmax_n(scale * q[t, h, :] . k[n, h, :]) . v[n, h, :] ) )
 * for t in [0, T), h in [0, H), n in [0, N), head dimension 128, no mask.  q is read in place (row stride ldq: the Q third of a packed
 * [T, 3 * H * 128] QKV buffer needs no copy); k and v are [N, H * 128] row-major with their own row strides -- what the adapter's
 * nn.Linear projections wrote; there is no transposed side input.  1 <= N <= 256 (K and V of one head stay in LDS; more keys:
 * SVDQ_E_UNSUPPORTED); any T >= 1, H >= 1.  Rows of k / v at or beyond N and rows of q / out at or beyond T are neither read nor
 * written.  q_prescaled: q already carries scale * log2(e) (svdq_gemm_args.q_scale) and `scale` is not applied again.
 * All scores of a row are formed before the softmax (one pass: max, exp2, sum); the probabilities are rounded to 16 bits before they
 * meet V and the row sum is taken over the rounded values, as in svdq_attention.  out_scale multiplies in fp32 (a 16-bit tensor times
 * a Python float in the reference: the scale itself is NOT rounded to 16 bits); out_scale == 1 yields round16(o).  The residual add of
 * the adapter is not part of this kernel: it is one svdq_residual_gate_stats pass (res + a, no gate), which also delivers the next
 * block's LayerNorm statistics.  No atomics, no workspace: two launches on the same inputs are bit-identical.
 * Validation (no launch): NULL pointers, N outside 1..256, T or H < 1, a row stride smaller than H * 128, pointers not 16-byte
 * aligned or strides not a multiple of 8 elements, unknown dtype, head_dim != 128 (SVDQ_E_UNSUPPORTED).
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_ip_attention_args {
    const void *q;   /* [T, H, 128] 16-bit, row stride ldq */
    const void *k;   /* [N, H * 128], row stride ldk */
    const void *v;   /* [N, H * 128], row stride ldv */
    void *out;       /* [T, H * 128], row stride ldo */
    int32_t ldq, ldk, ldv, ldo; /* in elements */
    int32_t T, H, N, head_dim;
    int32_t dtype;
    int32_t q_prescaled;
    float scale;     /* softmax scale (1 / sqrt(128) in the adapter); ignored with q_prescaled */
    float out_scale; /* fp32 */
} svdq_ip_attention_args;

/* Addressing reach:
 *   ldq, ldk, ldv, ldo  the field's width: (size_t)row * ld, (size_t)head * 128
 *   T, T * ld           int32 rows; 64-bit product        N  at most 256 (SVDQ_E_UNSUPPORTED)        H  at most 65535 (the grid) */
int svdq_ip_attention(const svdq_ip_attention_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * ReLU linear attention (SANA's LiteLA; added WITHOUT a version bump: two new symbols and a new args struct, nothing existing changes,
 * so SVDQ_ABI_VERSION stays 24.  reference: src/SanaModel.cpp:25-106, epilogues.cuh:552-761 -- there an epilogue of the QKV GEMM that
 * adds into vk with fp32 atomics, and a second kernel for the product with Q; here the QKV GEMM runs its plain epilogue and this call
 * reads the packed buffer it wrote, in place).  Per batch element b < B and head h < H, over the tokens t < T, head dimension 32:
 *   vk[b, h, i, j]  = sum_t V[t, i] * relu(K[t, j])      i, j < 32, fp32
 *   vk[b, h, 32, j] = sum_t relu(K[t, j])
 *   out[b, t, h, i] = round16( (sum_j relu(Q[t, j]) * vk[i, j]) / (sum_j relu(Q[t, j]) * vk[32, j] + eps) )
 * q is [T, H, 32] (head h at column 32 h of a row), kv is [T, H, 64] (K of head h at column 64 h, V at 64 h + 32: the order of the
 * reference's QKV projection behind its Q third), out is [T, H * 32] token-major; each has a row stride and a batch stride in
 * elements, so the thirds of a packed [B, T, 3 * H * 32] buffer are read in place.  Rows at or beyond T of a batch element are neither
 * read nor written; batch elements may start on any row.  vk (optional) receives the final sums.  q == NULL && out == NULL: only vk.
 * vk is fp32 from the matrix core's accumulator to the quotient (at T = 2100 a 16-bit vk overflows).
 * No atomics: the tokens are cut into chunks of 256, every chunk's [33, 32] fp32 partial goes to `workspace`, a finishing kernel adds
 * the partials in chunk order: two calls on the same inputs are bit-identical.  At most three kernel launches (two for vk alone), no
 * allocation, no synchronisation: the call can be captured.  workspace: svdq_linear_attention_workspace_bytes(args) bytes (depends on
 * B, H, T only), no zero fill needed, contents are scratch; reuse is allowed for calls ordered on one stream.
 * Validation (no launch): NULL args / kv / workspace, q without out or the reverse, neither and no vk, T / H / B < 1 (or beyond the
 * grid: H, B <= 65535, H * B <= 2^20, T <= 2^30), a row stride smaller than the row, a batch stride (B > 1) smaller than
 * (T - 1) * row stride + row width, pointers not 16-byte aligned or strides not a multiple of 8 elements, unknown dtype, eps negative
 * or not finite, a workspace smaller than the query says (svdq_last_error() names the byte count): SVDQ_E_INVALID;
 * head_dim != 32: SVDQ_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_linear_attention_args {
    const void *q;   /* [B][T, H, 32] 16-bit, row stride ldq, batch stride q_bs; NULL (with out): only vk */
    const void *kv;  /* [B][T, H, 64], row stride ldkv, batch stride kv_bs */
    void *out;       /* [B][T, H * 32], row stride ldo, batch stride out_bs */
    float *vk;       /* [B, H, 33, 32] fp32 contiguous, or NULL */
    void *workspace;
    int64_t workspace_bytes;
    int64_t q_bs, kv_bs, out_bs; /* in elements; ignored when B == 1 */
    int32_t ldq, ldkv, ldo;      /* in elements */
    int32_t B, T, H, head_dim;
    int32_t dtype;
    float eps;       /* 1e-6 in the reference */
    int32_t reserved;
} svdq_linear_attention_args;

/* Addressing reach:
 *   ldq, ldkv, ldo      the field's width: (size_t)row * ld
 *   q_bs, kv_bs, out_bs int64: (long long)b * bs
 *   T                   at most 2^30        H, B  at most 65535 each, H * B at most 2^20 (the grid)        T * ld, B * bs  64-bit products */
int svdq_linear_attention(const svdq_linear_attention_args *args, void *stream);
int64_t svdq_linear_attention_workspace_bytes(const svdq_linear_attention_args *args);

/* ------------------------------------------------------------------------------------------
 * Depthwise 3x3 convolution (SANA's GLU-MBConv; added WITHOUT a version bump: one new symbol and a new args struct, nothing existing
 * changes, so SVDQ_ABI_VERSION stays 24.  reference: DWCONV, src/Linear.cpp:542-551 -> dwconv_f16, src/kernels/dwconv.cu -- a CUTLASS
 * direct-convolution template; called between the two GEMMs of SanaGLUMBConv, src/SanaModel.cpp:192-213).
 * Cross-correlation, stride 1, zero padding 1, channels-last: x and out are [B][H * W, C] token rows -- the GEMM's [B * T, C] output
 * with T = H * W -- each with a row stride (per token) and a batch stride in elements, so each may be a column slice of a wider buffer.
 * Per element, in fp32 and in exactly this order (which makes a CPU restatement bit-equal):
 *   acc = bias[c] (or +0);  for ky = 0..2, for kx = 0..2:  acc += weight[ky * 3 + kx, c] * x[h + ky - 1, w + kx - 1, c];
 *   out[h, w, c] = round16(acc)        (round to nearest even, once)
 * A tap outside the image contributes the product with a zero, as conv2d's padding does.  The reference accumulates in the 16-bit
 * type (ElementAccumulator = half_t, dwconv.cu:223): nine roundings where this call has one.
 * weight is the TAP-MAJOR image [9, C] of the module's [C, 3, 3, 1] parameter (weight[ky * 3 + kx, c] = w[c, ky, kx, 0]: 8 channels
 * of a tap are one 16-byte load), in the activation dtype; bias [C] or NULL.
 * One launch, no workspace, no atomics, no allocation, no synchronisation: the call can be captured; two calls are bit-identical.
 * Nothing outside x[:, :H * W, :C] is read and nothing outside out[:, :H * W, :C] is written; every offset is formed in 64 bits.
 * Validation (no launch), SVDQ_E_INVALID: NULL args / x / weight / out, unknown dtype, B / H / W / C < 1, C % 8, a row stride below
 * C or not a multiple of 8, a batch stride (B > 1) below H * W * row stride or not a multiple of 8, pointers not 16-byte aligned,
 * x and out overlapping (in place is not supported), B > 65535 or more than 2^31 - 1 tiles.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_dwconv3x3_args {
    const void *x;      /* [B][H * W, C] 16-bit, row stride ldx, batch stride x_bs */
    const void *weight; /* [9, C] tap-major, contiguous */
    const void *bias;   /* [C] or NULL */
    void *out;          /* [B][H * W, C], row stride ldo, batch stride out_bs */
    int64_t x_bs, out_bs; /* in elements; ignored when B == 1 */
    int32_t ldx, ldo;     /* in elements */
    int32_t B, H, W, C;
    int32_t dtype;
    int32_t reserved;
} svdq_dwconv3x3_args;

/* Addressing reach:
 *   ldx, ldo            the field's width: ((long long)h * W + w) * ld
 *   x_bs, out_bs        int64: (long long)b * bs
 *   B                   at most 65535        ceil(C/512) * tiles of W * tiles of H  at most 2^31 - 1 (the grid)        H * W * ld, B * bs  64-bit products */
int svdq_dwconv3x3(const svdq_dwconv3x3_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Variable-length cross-attention (SANA's text cross-attention; added WITHOUT a version bump: one new symbol and a new args struct,
 * nothing existing changes, so SVDQ_ABI_VERSION stays 24.  reference: MultiHeadCrossAttention::forward, src/SanaModel.cpp:147-190 ->
 * flash-attention's mha_varlen_fwd).  Per sample b < B, query t < T and head h < H:
 *   out[b, t, h, :] = round16( softmax_n(scale * q[b, t, h, :] . k[n, h, :]) . v[n, h, :] )
 *   for n in [key_offsets[b], key_offsets[b] + key_counts[b])
 * q and out are [B * T, H * head_dim] token rows (sample b owns rows b * T .. b * T + T - 1) with row strides ldq / ldo, so each may be
 * a column slice of a wider buffer; k and v are [Nrows, H * head_dim] with row strides ldk / ldv -- the two column halves of one
 * [Nrows, 2 * H * head_dim] projection are read in place.  head_dim 72, 112 or 128 (anything else: SVDQ_E_UNSUPPORTED).
 * key_offsets and key_counts are DEVICE int32[B] and are read by the kernel only: no synchronisation, the call can be captured.  The
 * packed layout of flash-attention is offsets = cu[:-1], counts = cu[1:] - cu[:-1]; a padded [B, L, .] condition is offsets = b * L,
 * counts = mask.sum(1).  The kernel clamps what it read: a count below 0 acts as 0, a count above max_keys as max_keys, an offset
 * outside [0, Nrows) gives an empty range and a range is cut at Nrows.  A sample without keys gets zero rows.
 * max_keys is the host's upper bound on any count, 0 <= max_keys <= 320 (K and V of one sample and head stay in LDS, 160 KiB at
 * head_dim 128; more: SVDQ_E_UNSUPPORTED, no launch).
 * The keys are walked in chunks of 64 from the sample's first key with an online softmax (exp2 with scale * log2(e); the probabilities
 * are rounded to 16 bits before they meet V, the row sum is taken over the rounded values, the normalisation follows the last MFMA, as
 * in svdq_attention): a row's arithmetic depends on its own sample's keys only.  One launch, no atomics, no workspace: two launches
 * are bit-identical.  Rows of k / v outside every range, rows of q / out beyond B * T and columns beyond H * head_dim are neither read
 * nor written.
 * Validation (no launch), SVDQ_E_INVALID: NULL args or pointers, B / T / H < 1, max_keys or Nrows < 0, a row stride below
 * H * head_dim, pointers not 16-byte aligned (range arrays: 4-byte) or strides not a multiple of 8 elements, unknown dtype, a scale
 * that is not finite and positive, B * H > 65535 or T > 2^30.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_cross_attention_args {
    const void *q;   /* [B * T, H * head_dim] 16-bit, row stride ldq */
    const void *k;   /* [Nrows, H * head_dim], row stride ldk */
    const void *v;   /* [Nrows, H * head_dim], row stride ldv */
    void *out;       /* [B * T, H * head_dim], row stride ldo */
    const int32_t *key_offsets; /* device int32[B] */
    const int32_t *key_counts;  /* device int32[B] */
    int32_t ldq, ldk, ldv, ldo; /* in elements */
    int32_t B, T, H, head_dim;
    int32_t Nrows, max_keys;
    int32_t dtype;
    float scale;     /* head_dim^-0.5 in the reference */
} svdq_cross_attention_args;

/* Addressing reach:
 *   ldq, ldo            the field's width: (size_t)(b * T + row) * ld
 *   ldk, ldv            the field's width: (size_t)(key_offsets[b] + key) * ld
 *   B * H               at most 65535        T  at most 2^30 (the grid)        B * T, Nrows  int32; their products with ld are 64-bit */
int svdq_cross_attention(const svdq_cross_attention_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Batched attention at head dimension 64 (the self- and cross-attention of Stable Diffusion XL's transformer blocks; added WITHOUT a
 * version bump: one new symbol and a new args struct, nothing existing changes, so SVDQ_ABI_VERSION stays 24.  reference:
 * NunchakuSDXLFA2Processor, nunchaku/models/attention_processors/sdxl.py -- a chunk, three view / transpose copies and torch's SDPA).
 * Per sample b < B, head h < H, query t < T and keys n < N:
 *   out[b, t, h, :] = round16( softmax_n(scale * q[b, t, h, :] . k[b, n, h, :]) . v[b, n, h, :] )        head_dim = 64, no mask
 * q and out are [B][T, H * 64], k and v are [B][N, H * 64]; each has a row stride (ldq / ldk / ldv / ldo) and a batch stride (q_bs / k_bs /
 * v_bs / out_bs; ignored at B = 1), all in elements: the three column thirds of a packed [B, T, 3 * H * 64] QKV projection (N = T) and the
 * [B, 77, H * 64] outputs of to_k / to_v are read in place, out is written token-major.  No transposed side input, no workspace, no
 * atomics, no synchronisation: the call can be captured and two launches are bit-identical.
 * The keys are walked in chunks of 64 from key 0 with an online softmax (exp2 with scale * log2(e); the probabilities are rounded to 16
 * bits before they meet V, the row sum is taken over the rounded values, the normalisation follows the last MFMA, as in svdq_attention
 * and svdq_cross_attention): a row's result depends on its own sample's and head's keys only.  Rows of k / v at or beyond N, rows of
 * q / out at or beyond T and columns beyond H * 64 are neither read nor written.
 * Validation (no launch), SVDQ_E_INVALID: NULL args or pointers, B / T / H / N < 1, B * H > 65535, T or N > 2^30, a row stride below
 * H * 64 or not a multiple of 8, a batch stride (B > 1) below (rows - 1) * ld + H * 64 or not a multiple of 8, pointers not 16-byte
 * aligned, unknown dtype, a scale that is not finite and positive, out overlapping an input.  SVDQ_E_UNSUPPORTED: head_dim != 64.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_attention_d64_args {
    const void *q;   /* [B][T, H * 64] 16-bit, row stride ldq, batch stride q_bs */
    const void *k;   /* [B][N, H * 64], row stride ldk, batch stride k_bs */
    const void *v;   /* [B][N, H * 64], row stride ldv, batch stride v_bs */
    void *out;       /* [B][T, H * 64], row stride ldo, batch stride out_bs */
    int64_t q_bs, k_bs, v_bs, out_bs; /* in elements; ignored at B = 1 */
    int32_t ldq, ldk, ldv, ldo;       /* in elements */
    int32_t B, T, H, N;
    int32_t head_dim; /* 64 */
    int32_t dtype;
    float scale;      /* 64^-0.5 in the reference */
    int32_t reserved;
} svdq_attention_d64_args;

/* Addressing reach:
 *   ldq, ldk, ldv, ldo  the field's width: (size_t)row * ld
 *   q_bs, k_bs, v_bs, out_bs   int64: (size_t)b * bs
 *   B * H               at most 65535        T, N  at most 2^30 (the grid)        T * ld, N * ld, B * bs  64-bit products */
int svdq_attention_d64(const svdq_attention_d64_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * SANA block glue (the element-wise passes between the three layers of a SANA block; added WITHOUT a version bump: one new symbol and a
 * new args struct, nothing existing changes, so SVDQ_ABI_VERSION stays 24.  reference: SanaLinearTransformerBlock::forward,
 * src/SanaModel.cpp:234-322 -- a copy of timestep, one add of scale_shift_table, two LayerNorms and five mul_add_batch launches per block;
 * here one row pass does the gated residual, the LayerNorm of the result, the next layer's per-sample modulation and the padding to the
 * GEMM operand width).  Rows are B * T tokens, row r belongs to sample b = r / T.  round16 = round to nearest even to `dtype`;
 * clip = min(max(., -65504), 65504) for SVDQ_FP16 and the identity for SVDQ_BF16 (mul_add_kernel, misc_kernels_impl.cuh:60-63); everything
 * between two roundings is fp32:
 *   mod(tab, i)[b, c] = clip(round16(timestep[b, i, c] + tab[i, c]))
 *   t = res                                                      (a NULL)
 *   t = clip(round16(a + res))                                   (a given, gate_row < 0: the cross-attention residual)
 *   t = clip(round16(round16(a * g) + res)),  g = mod(gate_table, gate_row)[b]
 *   out[r, :C] = t;  out[r, C:C_pad] = +0                        (if out)
 *   mean, rstd = the two-pass fp32 statistics of the C stored values t, formed as svdq_residual_gate_stats forms them
 *   stats[r] = (mean, rstd)                                      (if stats)
 *   n = round16((t - mean) * rstd)
 *   s = round16(mod(mod_table, scale_row)[b] + 1);  h = mod(mod_table, shift_row)[b]
 *   out_mod[r, :C] = clip(round16(round16(n * s) + h));  out_mod[r, C:C_pad] = +0       (if out_mod)
 * These are the rounding points of the reference's SEPARATE operations (SanaModel.cpp:255,272,278,292,304,310;
 * layernorm_kernels_impl.cuh:14,132).  nvcc is free to contract the reference's `x * (scale + 1) + bias` into one fma, which drops the
 * rounding of the product; this project fixes the reading above (the library is built with -ffp-contract=off).
 * gate_table and mod_table are separate [6, C] tables: the pass behind the feed-forward gates with its own block's table and modulates
 * with the next block's.  timestep is [B, 6, C] with batch stride timestep_bs (elements), row i of a sample C elements behind row i - 1.
 * Every tensor has its own row stride (a is the first C columns of a C_pad-wide GEMM output).  C % 8 == 0, C <= C_pad, C_pad % 8 == 0,
 * ceil(C_pad / 512) in {1..8, 12, 16, 24, 32} (else SVDQ_E_UNSUPPORTED).  out may alias res when ld_out == ld_res; out_mod may alias nothing
 * that is read.  Nothing is read outside res[:, :C], a[:, :C], the two tables and the rows of timestep[b] that are used; nothing is written
 * outside the C_pad columns of the two outputs or past row B * T.  One launch, no workspace, no atomics, no synchronisation: the call can
 * be captured and two calls on the same inputs are bit-identical.
 * Validation (no launch), SVDQ_E_INVALID: NULL args or res, none of out / out_mod / stats, a gate row without a, a gate / scale / shift row
 * outside 0..5, out_mod without timestep or mod_table, a gate without timestep or gate_table, B / T / C < 1, C > C_pad, a stride smaller
 * than its row, pointers not 16-byte aligned (stats: 8-byte) or a stride that is not a multiple of 8, unknown dtype, an eps that is
 * negative or not finite, B * T > 2^31 - 1.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_sana_glue_args {
    const void *res;        /* [B * T, C] 16-bit, row stride ld_res */
    const void *a;          /* [B * T, C], row stride ld_a, or NULL */
    const void *timestep;   /* [B, 6, C], batch stride timestep_bs; NULL when neither a gate nor out_mod is asked for */
    const void *gate_table; /* [6, C] contiguous, or NULL (no gate) */
    const void *mod_table;  /* [6, C] contiguous, or NULL (no out_mod) */
    void *out;              /* [B * T, C_pad], row stride ld_out, or NULL */
    void *out_mod;          /* [B * T, C_pad], row stride ld_mod, or NULL */
    float *stats;           /* [B * T, 2] fp32 or NULL */
    int64_t timestep_bs;    /* in elements, >= 6 * C, a multiple of 8 */
    int32_t ld_res, ld_a, ld_out, ld_mod; /* in elements */
    int32_t B, T, C, C_pad;
    int32_t gate_row;       /* 0..5, or < 0: no gate */
    int32_t scale_row, shift_row; /* 0..5 (looked at only with out_mod) */
    int32_t dtype;
    float eps;
    int32_t reserved;
} svdq_sana_glue_args;

/* Alignment of the operands of svdq_sana_glue ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   res, a, timestep, gate_table, mod_table, out, out_mod  16 bytes
 *   stats                                                  8 bytes
 *   ld_res, ld_a, ld_out, ld_mod, timestep_bs              8 elements */
/* Addressing reach:
 *   ld_res, ld_a, ld_out, ld_mod   the field's width: (size_t)row * ld
 *   timestep_bs         int64: 64-bit sample offset
 *   B * T, B * T * ld   int32 rows; 64-bit product */
int svdq_sana_glue(const svdq_sana_glue_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Z-Image block glue, part 1: the sandwich norm (added WITHOUT a version bump: one new symbol and a new args struct, nothing existing
 * changes, so SVDQ_ABI_VERSION stays 24.  reference: diffusers' ZImageTransformerBlock as nunchaku/models/transformers/transformer_zimage.py
 * patches it -- four full-width RMSNorms around the two sub-layers, two per-sample modulations, two tanh-gated residuals, each a 16-bit torch
 * operation).  One row pass closes a sub-layer and opens the next.  Rows are M = B * T tokens, row r belongs to sample b = r / T.
 * round16 = round to nearest even to `dtype`; every operation between two roundings is ONE plain fp32 multiply or add whose fp32 result is
 * then rounded to 16 bits (no fused multiply-add, no fp16 clipping):
 *   rstd(h) = 1 / sqrt(sum_c(h[c]^2) / C + eps);      rms(h, w)[c] = round16(round16(h[c] * rstd(h)) * w[c])
 *   y = res                                                                          (a NULL)
 *   y = round16(res + rms(a, w_post))                                                (a given, gate NULL)
 *   y = round16(res + round16(gate[b] * rms(a, w_post)))                             (a and gate given)
 *   out[r] = y                                                                       (if out)
 *   out_mod[r] = rms(y, w_pre)  |  round16(rms(y, w_pre) * scale[b])                 (if out_mod; scale NULL | given)
 *   stats[r] = (rstd(a) or 0 without a, rstd(y))                                     (if stats)
 * The sums of squares run in one fixed order (a lane adds its elements in index order, a 6-level butterfly folds the wave), so two calls
 * are bit-identical; a term passes through at most 8 * ceil(C / 512) + 6 additions.  gate and scale are [B, C] with batch strides gate_bs /
 * scale_bs (elements); they hold what the block applies, i.e. tanh(gate) and 1 + scale.  Every tensor of rows has its own row stride.
 * C % 8 == 0, ceil(C / 512) in {1..8, 12, 16, 24, 32} (else SVDQ_E_UNSUPPORTED).  out may alias res when ld_out == ld_res; out_mod may alias
 * nothing that is read.  One launch, no workspace, no LDS, no atomics: the call can be captured.
 * Validation (no launch), SVDQ_E_INVALID: NULL args or res, none of out / out_mod / stats, gate without a, a without w_post, out_mod
 * without w_pre, M or C < 1, C % 8, a row stride below C or not a multiple of 8, T < 1 or M % T, a batch stride below C or not a multiple
 * of 8, pointers not 16-byte aligned (stats: 8-byte), unknown dtype, an eps that is negative or not finite.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_sandwich_norm_args {
    const void *res;    /* [M, C] 16-bit, row stride ld_res */
    const void *a;      /* [M, C], row stride ld_a: the sub-layer's output, or NULL */
    const void *w_post; /* [C]: the RMSNorm weight behind the sub-layer (with a) */
    const void *gate;   /* [B, C], batch stride gate_bs, or NULL */
    const void *w_pre;  /* [C]: the RMSNorm weight in front of the next sub-layer (with out_mod) */
    const void *scale;  /* [B, C], batch stride scale_bs, or NULL */
    void *out;          /* [M, C], row stride ld_out, or NULL */
    void *out_mod;      /* [M, C], row stride ld_mod, or NULL */
    float *stats;       /* [M, 2] fp32 or NULL */
    int64_t gate_bs, scale_bs;            /* in elements */
    int32_t ld_res, ld_a, ld_out, ld_mod; /* in elements */
    int32_t M, T, C, dtype;
    float eps;
    int32_t reserved;
} svdq_sandwich_norm_args;

/* Alignment of the operands of svdq_sandwich_norm ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   res, a, w_post, gate, w_pre, scale, out, out_mod  16 bytes
 *   stats                                             8 bytes
 *   ld_res, ld_a, ld_out, ld_mod, gate_bs, scale_bs   8 elements */
/* Addressing reach:
 *   ld_res, ld_a, ld_out, ld_mod   the field's width: (size_t)row * ld
 *   gate_bs, scale_bs   int64: b * (size_t)bs
 *   M, M * ld           int32 rows; 64-bit product */
int svdq_sandwich_norm(const svdq_sandwich_norm_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Z-Image block glue, part 2: per-head RMSNorm of Q and K, RoPE and V^T (added WITHOUT a version bump, as above.  reference:
 * NunchakuZSingleStreamAttnProcessor, nunchaku/models/attention_processors/zimage.py:35-88 -- two RMSNorms over head_dim, a rotation
 * through fp32 complex tensors, three unflatten / transpose copies into SDPA).  One sample per launch.  qkv is the packed
 * [T, 3 * H * 128] output of the QKV projection (row stride ld): Q of head h at column h * 128, K at H * 128 + h * 128, V at
 * 2 * H * 128 + h * 128.  The Q and K thirds are rewritten IN PLACE, per token t and head, on the 128 values x of Q and of K:
 *   n = round16(round16(x * rstd) * w),  rstd = 1 / sqrt(sum(x^2) / 128 + eps),  w = norm_q | norm_k [128]         (w NULL: n = x)
 *   x'[2i] = round16(n[2i] * c - n[2i+1] * s),  x'[2i+1] = round16(n[2i] * s + n[2i+1] * c),  (c, s) = freqs[t, i]   (freqs NULL: x' = n)
 * with plain fp32 multiplies, adds and subtractions between the roundings (no fused multiply-add).  freqs is [T, 64, 2] fp32 (cos, sin):
 * torch.view_as_real of the pipeline's complex freqs_cis.  V is not changed; with vt, vt[h * 128 + d, t] = V[t, h * 128 + d] for t < T
 * and +0 for T <= t < L_pad (svdq_attention needs finite V^T under masked keys); nothing is written at or beyond column L_pad.
 * rstd (optional): [T, 2 * H] fp32, column h for Q and H + h for K of head h (0 where there is no norm).  No atomics; two calls on the
 * same input are bit-identical.
 * Validation (no launch), SVDQ_E_INVALID: NULL args or qkv, T < 1, H < 1 or > 65535, ld < 3 * H * 128 or not a multiple of 8, with vt:
 * L_pad < T or not a multiple of 128, ldvt < L_pad or not a multiple of 8; pointers not 16-byte aligned (rstd: 4-byte), unknown dtype, an
 * eps that is negative or not finite.  head_dim != 128: SVDQ_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_qk_norm_rope_args {
    void *qkv;          /* [T, 3 * H * 128] 16-bit, row stride ld */
    const void *norm_q; /* [128] 16-bit or NULL */
    const void *norm_k; /* [128] 16-bit or NULL */
    const float *freqs; /* [T, 64, 2] fp32 or NULL */
    void *vt;           /* [H * 128, ldvt] 16-bit or NULL */
    float *rstd;        /* [T, 2 * H] fp32 or NULL */
    int32_t ld, ldvt;   /* in elements */
    int32_t T, L_pad, H, head_dim;
    int32_t dtype;
    float eps;
} svdq_qk_norm_rope_args;

/* Alignment of the operands of svdq_qk_norm_rope ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   qkv, norm_q, norm_k, freqs, vt  16 bytes
 *   rstd                            4 bytes
 *   ld, ldvt                        8 elements */
/* Addressing reach:
 *   ld                  the field's width: (size_t)t * ld
 *   ldvt                the field's width: (size_t)(h * 128 + d) * ldvt
 *   H                   at most 65535 (the grid)        T, L_pad  int32; T * ld and H * 128 * ldvt are 64-bit products */
int svdq_qk_norm_rope(const svdq_qk_norm_rope_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Qwen-Image rotary tables for one or several latent grids (added WITHOUT a version bump: one new symbol and a new args struct, nothing
 * existing changes, so SVDQ_ABI_VERSION stays 24.  reference: diffusers QwenEmbedRope.forward / _compute_video_freqs, as the Edit pipelines
 * call it with img_shapes = [[(1, h, w), (1, h1, w1), ...]] -- the noise latents and one to three reference images).  One launch writes
 * what nunchaku_amd/models/qwenimage.py pack_qwen_rotary returns, gathered from two per-axis tables that depend on theta and axes_dim only:
 *   pos_cs[k, c] = (cos, sin)(float(k) * inv[c])          k = 0 .. 4095, c = 0 .. 63
 *   neg_cs[k, c] = (cos, sin)(float(-(k + 1)) * inv[c])   row k holds position -(k + 1)
 * with the channels of the frame, height and width axes side by side: [0, c_frame), [c_frame, c_frame + c_height), the rest.
 * Image rows: the grids back to back, grid g (0-based, extents (F, H, W)) flattened frame-major, then height, then width.  Row (f, h, w) of
 * grid g reads position g + f on the frame axis, h - (H - H / 2) on the height axis with scale_rope (h without) and w - (W - W / 2) (w) on the
 * width axis.  Text row t reads position txt_start + t on all three axes (diffusers: txt_start = max over the grids of max(H / 2, W / 2)
 * with scale_rope, of max(H, W) without -- the caller's rule, not the library's).
 * Outputs (each optional; NULL skips it; all fp32).  T = the image rows, pad(n) = n rounded up to 256:
 *   img [pad(T), 128], txt [pad(txt_len), 128], all [pad(txt_len) + pad(T), 128]: (sin, cos) in the QKV epilogue's order (svdq_gemm_args.rotary_emb,
 *       models/embeddings.py pack_rotemb); `all` is the joint sequence [text | image] with each stream on a 256-row boundary
 *   img_cs [T, 64, 2], txt_cs [txt_len, 64, 2]: plain (cos, sin)
 * Rows at or beyond a stream's length are +0, the gap between the padded text and the image in `all` included: every byte of every given
 * output is written (callers pass uninitialised memory).  Pure data movement -- bit-equal to the torch sequence on the same axis tables; no
 * atomics; 16-byte stores, consecutive lanes consecutive addresses.
 * Validation (no launch), SVDQ_E_INVALID: NULL args, NULL pos_cs or neg_cs, no output given; count outside 1 .. 8; an extent below 1;
 * a position the launch would read at or beyond 4096 (g + F > 4096; max(H, W) - max(H, W) / 2 > 4096 with scale_rope, max(H, W) > 4096
 * without; txt_start + txt_len > 4096); txt_len or txt_start negative; c_frame / c_height negative or more than 64 together; a pointer
 * that is not 16-byte aligned; more than 33554432 rows (see the reach below).
 * ------------------------------------------------------------------------------------------ */
#define SVDQ_QWEN_ROTARY_MAX_GRIDS 8
#define SVDQ_QWEN_ROTARY_POSITIONS 4096
#define SVDQ_QWEN_ROTARY_MAX_ROWS 33554432
typedef struct svdq_qwen_rotary_args {
    const float *pos_cs;  /* [4096, 64, 2] fp32 */
    const float *neg_cs;  /* [4096, 64, 2] fp32 */
    float *img, *txt, *all, *img_cs, *txt_cs;
    int32_t grids[3 * SVDQ_QWEN_ROTARY_MAX_GRIDS]; /* (F, H, W) of grid 0, grid 1, ...: by value */
    int32_t count;        /* grids in use, 1 .. 8 */
    int32_t txt_len;      /* text rows (0: the text tables are empty, `all` is the image alone) */
    int32_t txt_start;    /* position of text row 0 */
    int32_t scale_rope;   /* non-zero: height and width positions centred */
    int32_t c_frame, c_height; /* channels (complex entries) of the frame and the height axis: 8 and 28 for axes_dim (16, 56, 56) */
} svdq_qwen_rotary_args;

/* Alignment of the operands of svdq_qwen_rotary: a pointer that is no multiple of its line is refused with SVDQ_E_INVALID before anything is
 * launched; NULL counts as aligned.
 *   pos_cs, neg_cs, img, txt, all, img_cs, txt_cs  16 bytes (the outputs are stored in 16-byte pieces; the tables are read in 8-byte pairs) */
/* Addressing reach:
 *   rows                a work item is one 16-byte piece and its index a 32-bit unsigned: at most 96 pieces per padded row over the five
 *                       outputs, so pad(T) + pad(txt_len) <= 33554432 (96 * 2^25 < 2^32); beyond: SVDQ_E_INVALID.  Byte offsets are 64-bit */
int svdq_qwen_rotary(const svdq_qwen_rotary_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * Folded identity cross-attention (PuLID for FLUX; added WITHOUT a version bump: one new symbol and a new args struct, nothing existing
 * changes, so SVDQ_ABI_VERSION stays 24.  reference: PerceiverAttentionCA, nunchaku/models/pulid/encoders_transformer.py:62-128 -- two
 * LayerNorms, to_q, to_kv, a 16-bit softmax and to_out in torch ops, called from FluxModel.cpp's residual_callback).  K and V depend on the
 * identity embeddings only, so to_q and to_out are folded into them once per embeddings tensor (nunchaku_amd/models/pulid.py): an attention
 * whose H heads share one query, the hidden row itself, over J = H * 32 folded keys a_fold and values b_fold, summed over the heads.
 * Per row t < T, head h < H, key n < N of the head (column j = 32 h + n; columns with n >= N take no part) and channel c < C:
 *   acc[t, j] = sum_c x[t, c] * a_fold[j, c]                         fp32, on the 16-bit matrix core, in a fixed order
 *   s[t, j]   = rstd_t * (acc[t, j] - mean_t * colsum[j]) + cbias[j]  (mean_t, rstd_t) = stats[t]; one fp32 rounding per operation
 *   P[t, j]   = round16( e_j / sum_n e_n ),  e_j = exp(s[t, j] - max_n s[t, n])    over the head's N keys, fp32; P = +0 for n >= N
 *   o[t, c]   = sum_j P[t, j] * b_fold[j, c]                         fp32, on the 16-bit matrix core
 *   out[t, c] = round16( out_scale * round16(o[t, c]) )              svdq_ip_attention's output rule: out_scale multiplies in fp32
 * This is the reference's softmax(weight.float()).type(dtype) with the LayerNorm of the query inside the score epilogue.  exp is formed from
 * plain fp32 operations (range reduction by ln 2 in two pieces, a degree-7 polynomial; exp of less than -80 is +0) and the sum runs in a fixed
 * order (nunchaku_amd/csrc/pulid_ca.hip), so the two epilogues can be restated bit for bit from acc and o (tests/pulid_ref.py).
 * probs [T, H * 32] is a 16-bit workspace that receives P (contents are a result: callers may read it).  acc / o_acc (optional, fp32,
 * contiguous [T, H * 32] / [T, C]) receive the two accumulators as the epilogues saw them.  Two kernel launches, no atomics, no allocation, no
 * synchronisation: the call can be captured, two calls are bit-identical, and a row's result depends on neither T nor the row's position.
 * Rows of a_fold / b_fold with n >= N, rows of x / stats at or beyond T and columns at or beyond C are never read; nothing is written
 * outside out[:T, :C], probs, acc and o_acc.
 * Validation (no launch), SVDQ_E_INVALID: NULL args or a missing pointer, T / C / H / N < 1, a row stride below C or not a multiple of 8,
 * pointers not 16-byte aligned (stats: 8-byte), unknown dtype, an out_scale that is not finite, more tiles than the grid holds.
 * SVDQ_E_UNSUPPORTED: C not a multiple of 128, H not a multiple of 4, H * 32 > 512, N > 32.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_pulid_ca_args {
    const void *x;       /* [T, C] 16-bit, row stride ldx */
    const float *stats;  /* [T, 2] fp32: (mean, rstd) of every row of x, eps = 1e-5 */
    const void *a_fold;  /* [H * 32, C] 16-bit, contiguous: key-major folded keys */
    const float *colsum; /* [H * 32] fp32: the sum over c of the 16-bit a_fold[j, c] */
    const float *cbias;  /* [H * 32] fp32 */
    const void *b_fold;  /* [H * 32, C] 16-bit, contiguous: folded values */
    void *probs;         /* [T, H * 32] 16-bit, contiguous: workspace, receives P */
    void *out;           /* [T, C] 16-bit, row stride ldo */
    float *acc;          /* [T, H * 32] fp32 or NULL */
    float *o_acc;        /* [T, C] fp32 or NULL */
    int32_t ldx, ldo;    /* in elements */
    int32_t T, C, H, N;
    int32_t dtype;
    float out_scale;     /* fp32 */
} svdq_pulid_ca_args;

/* Alignment of the operands of svdq_pulid_ca ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   x, a_fold, colsum, cbias, b_fold, probs, out, acc, o_acc  16 bytes
 *   stats                                                     8 bytes
 *   ldx, ldo                                                  8 elements */
/* Addressing reach:
 *   ldx, ldo            the field's width: (size_t)row * ld
 *   T, T * ld, T * H * 32   int32 rows; 64-bit products */
int svdq_pulid_ca(const svdq_pulid_ca_args *args, void *stream);

/* ------------------------------------------------------------------------------------------
 * AWQ W4A16 GEMV (reference: ops.gemv_awq, nunchaku/csrc/ops.h:123-145 -> src/kernels/awq/gemv_awq.cu:100-286;
 * module nunchaku/models/linear.py:277-414).  The AdaLayerNormZero modulation projections of every block.
 *   out[m, n] = round16( sum_k round16( round16(q[n,k]*scales[k/64,n] + zeros[k/64,n]) * x[m,k] ) ) (+ bias[n])
 * qweight is the CHECKPOINT tensor as stored ([N/4, K/2] int32, tinychat pack_w4 order,
 * text_encoders/tinychat_utils.py:76-107) -- no load-time repack.  scales / zeros are [K/64, N] 16-bit,
 * zeros already scaled and negated (w = q*scale + zeros).  1 <= M <= 8 as in the reference.
 * bias (optional, [N] 16-bit) fuses AWQW4A16Linear.forward's output.add_(bias) (one more 16-bit rounding).
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_gemv_awq_args {
    const void *x;        /* [M, K] 16-bit, row stride ldx */
    const void *qweight;  /* [N/4, K/2] int32 */
    const void *scales;   /* [K/64, N] 16-bit, 2-byte aligned as zeros, bias and out */
    const void *zeros;    /* [K/64, N] 16-bit */
    const void *bias;     /* [N] 16-bit or NULL */
    void *out;            /* [M, N] 16-bit, contiguous */
    int32_t M, N, K, ldx;
    int32_t group_size;   /* must be 64 */
    int32_t dtype;        /* SVDQ_BF16 | SVDQ_FP16 */
    int32_t out_chunks;   /* 0 / 1: natural out[m, n].  c > 1 (N % c == 0): de-interleaved, element n is written to
                             out[m, (n % c) * (N / c) + n / c] -- the modulation vectors of AdaLayerNormZero are stored
                             interleaved per channel (emb.view(B, -1, 6).permute(2, 0, 1), normalization.py:89) and come
                             out as c contiguous [N/c] vectors */
    int32_t reserved;
} svdq_gemv_awq_args;

/* Alignment of the operands of svdq_gemv_awq and svdq_gemv_awq_batched ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   x, qweight                16 bytes
 *   scales, zeros, bias, out  2 bytes
 *   ldx                       8 elements */
/* Addressing reach:
 *   ldx                 the field's width: (size_t)m * ldx, M at most 8 (svdq_gemv_awq_batched: M = 1, ldx is not multiplied)
 *   N * K               the packed weight is indexed in 64 bits */
int svdq_gemv_awq(const svdq_gemv_awq_args *args, void *stream);
/* `count` (<= 80) independent GEMVs that share x, M, K, dtype and group_size in ONE launch (extension): all the
 * modulation projections of a denoising step depend only on the timestep embedding, so they can be issued together
 * before the first block instead of one launch per block.  Each entry brings its own qweight / scales / zeros / bias /
 * out / N / out_chunks; x, M, K, ldx, group_size and dtype are taken from args[0]. */
#define SVDQ_GEMV_BATCH_MAX 80
int svdq_gemv_awq_batched(const svdq_gemv_awq_args *args, int32_t count, void *stream);

/* Low-rank (LoRA) branch of the M = 1 GEMV (reference: GEMV_AWQ lora_down / lora_up / lora_scale, src/Linear.cpp): `count`
 * (<= SVDQ_GEMV_BATCH_MAX) layers in one call, issued behind svdq_gemv_awq_batched on the same stream over the entries that
 * carry a LoRA.  Per entry, with fp32 accumulation and three 16-bit roundings:
 *   t[j]    = round16( sum_k down[j,k] * x[k] )
 *   d[n]    = round16( strength * sum_j up[n,j] * t[j] )
 *   out[n'] = round16( out[n'] + d[n] ),  n' = (n % c) * (N / c) + n / c for out_chunks = c > 1 (the layout the GEMV wrote), else n
 * (the sums and the product with strength are formed in fp64 and rounded once to 16 bits: each rounding point is the correctly rounded value.)
 * r must be a multiple of 16, 16 <= r <= 128 (zero-pad the factors), K a multiple of 8; x, K and dtype are shared by all
 * entries; x, down and up 16-byte aligned.  Two kernels (down, then up), no host synchronisation, safe under stream capture.
 * Every t[j] and every out[n'] has one owner with a fixed summation order -- no atomics: bit-reproducible.  An update that
 * rounds to zero (strength = 0) leaves out bit for bit as it was.  `t` must not be shared between entries of one call. */
typedef struct svdq_gemv_lora_args {
    const void *x;      /* [K] 16-bit: the GEMV's input row */
    const void *down;   /* [r, K] 16-bit, row-major */
    const void *up;     /* [N, r] 16-bit, row-major (logical output order: NOT de-interleaved) */
    void *out;          /* [N] 16-bit, read-modify-write */
    void *t;            /* [r] 16-bit scratch: the down projection, written by the first kernel and read by the second */
    float strength;
    int32_t r, N, K;
    int32_t dtype;      /* SVDQ_BF16 | SVDQ_FP16 */
    int32_t out_chunks; /* as svdq_gemv_awq_args.out_chunks */
    int32_t reserved[2];
} svdq_gemv_lora_args;

/* Alignment of the operands of svdq_gemv_awq_lora_batched ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   x, down, up  16 bytes
 *   out, t       2 bytes */
int svdq_gemv_awq_lora_batched(const svdq_gemv_lora_args *entries, int32_t count, void *stream);

/* ------------------------------------------------------------------------------------------
 * AWQ W4A16 GEMM, group 128 (ABI 23; reference: ops.gemm_awq, nunchaku/csrc/ops.h:148-160 -> src/kernels/awq/gemm_awq.cu;
 * module nunchaku/models/text_encoders/linear.py, W4Linear).  The projections of the 4-bit T5 text encoder, any M >= 1.
 *   w16[n, k] = round16( fma(q[n,k], scales[k/128, n], scaled_zeros[k/128, n]) )     one 16-bit rounding (__hfma2)
 *   out[m, n] = round16( sum_k w16[n,k] * x[m,k] )                                    exact products, fp32 sums (MFMA)
 *   (+ bias[n], optional: one more 16-bit rounding, W4Linear.forward's `out + bias`)
 * qweight is the CHECKPOINT tensor as stored: [N/4, K] int16 (the same bytes as the GEMV's [N/4, K/2] int32), tinychat
 * pack_w4 order -- no load-time repack.  scales / scaled_zeros are [G_pad, N] 16-bit with G_pad >= K/128 (the converter
 * pads G_pad to ceil_num_groups; rows >= K/128 are not read).  K % 128 == 0, N % 64 == 0, group_size == 128 (else
 * SVDQ_E_UNSUPPORTED).  fp16 outputs beyond the range go to +-inf (round to nearest, no clamp), as in the reference.
 * K-split: a launch whose output tiles do not fill the chip splits K into slices; each slice stores fp32 partial tiles into
 * `workspace` and a second kernel adds them in slice order (bit-identical from launch to launch).  workspace = NULL: no
 * split (same contract, another fp32 summation order); a non-NULL workspace must hold svdq_gemm_awq_workspace_bytes(M, N, K)
 * bytes (16-byte aligned; no zero fill needed), else SVDQ_E_INVALID.  The plan depends on (M, N, K) only, not on the device.
 * ------------------------------------------------------------------------------------------ */
typedef struct svdq_gemm_awq_args {
    const void *x;            /* [M, K] 16-bit, row stride ldx (>= K, % 8 == 0), 16-byte aligned */
    const void *qweight;      /* [N/4, K] int16, 16-byte aligned */
    const void *scales;       /* [G_pad, N] 16-bit */
    const void *scaled_zeros; /* [G_pad, N] 16-bit (zeros already scaled and negated: w = q*scale + scaled_zero) */
    const void *bias;         /* [N] 16-bit or NULL */
    void *out;                /* [M, N] 16-bit, contiguous, 8-byte aligned (the K-split's second kernel stores four elements at a time) */
    void *workspace;          /* fp32 partial tiles of the K-split, or NULL */
    int64_t workspace_bytes;
    int32_t M, N, K, ldx;
    int32_t group_size;       /* must be 128 */
    int32_t dtype;            /* SVDQ_BF16 | SVDQ_FP16 */
} svdq_gemm_awq_args;

/* Alignment of the operands of svdq_gemm_awq ("Alignment").  A pointer or stride that is no multiple of its line is
 * refused with SVDQ_E_INVALID before anything is launched; NULL counts as aligned.  tests/test_alignment_contract.py holds the widest access behind every line:
 *   x, qweight, workspace       16 bytes
 *   out                         8 bytes: the K-split's second kernel stores four elements at a time
 *   scales, scaled_zeros, bias  2 bytes
 *   ldx                         8 elements */
/* Addressing reach:
 *   ldx                 the field's width: (size_t)row * ldx
 *   M, M * ldx, M * N   int32 rows; 64-bit products */
int svdq_gemm_awq(const svdq_gemm_awq_args *args, void *stream);
/* workspace bytes a launch of this shape uses (0: it does not split K) */
int64_t svdq_gemm_awq_workspace_bytes(int32_t M, int32_t N, int32_t K);

/* ------------------------------------------------------------------------------------------
 * Load-time re-layout of reference checkpoint tensors (NVIDIA fragment order -> CDNA4 order).
 * src and dst must not alias.  All but svdq_repack_qweight (4 -> 6 bits per code) and svdq_repack_wscales (x 32) are pure permutations of equal size.
 * ------------------------------------------------------------------------------------------ */
/* qweight [N, K/2] int8 (packer.py:187-239) -> FP6 image, N*K*3/4 bytes, consumed by svdq_gemm_w4a4 */
int svdq_repack_qweight(const void *src, void *dst, int32_t N, int32_t K, void *stream);
/* wscales [K/64, N] 16-bit (packer.py:241-301) -> scale image [N/32][K/128][2][32]; G must be even.  ABI 21: takes the dtype, and the image holds 32 x the
 * scale: the GEMM's product MFMA runs without MX block scales (P = dot / 64), the scale tile is S = 2 ws' as, and ws' = 32 ws makes P S the fp32 product of
 * the ABI 20 kernels bit for bit.  Exact for bf16; an fp16 scale above 2047 overflows to inf (weights beyond 14 000) -- svdq_unrepack_wscales divides again. */
int svdq_repack_wscales(const void *src, void *dst, int32_t G, int32_t N, int32_t dtype, void *stream);
/* bias / smooth_factor [N] 16-bit (same intra-128 permutation, gemm_base.cuh:713) -> natural */
int svdq_repack_vec(const void *src, void *dst, int32_t N, void *stream);
/* proj_up [N, R] (down=0) -> natural [n][r];  proj_down [K, R] (down=1) -> [r][k] (rank-major)
 * (packer.py:362-398, lora.cuh:43-59).  C = N or K. */
int svdq_repack_lowrank(const void *src, void *dst, int32_t C, int32_t R, int32_t down, void *stream);

/* Inverse re-layouts (kernel order -> the reference's checkpoint order): what state_dict() of a repacked layer returns and
 * what the host-offload manager keeps in pinned memory (4-bit nibbles: 2/3 of the FP6 image's bytes on the PCIe link).
 * Exact inverses of svdq_repack_*: repack(unrepack(x)) == x and unrepack(repack(c)) == c bit for bit. */
int svdq_unrepack_qweight(const void *src, void *dst, int32_t N, int32_t K, void *stream); /* FP6 image -> [N, K/2] int8 */
int svdq_unrepack_wscales(const void *src, void *dst, int32_t G, int32_t N, int32_t dtype, void *stream);
int svdq_unrepack_vec(const void *src, void *dst, int32_t N, void *stream);
int svdq_unrepack_lowrank(const void *src, void *dst, int32_t C, int32_t R, int32_t down, void *stream);

/* Inverse helpers used by the tests to read the opaque formats back:
 * FP6 image -> one int8 code per element, natural [ROWS, K];  scale image -> natural [G][ROWS]. */
int svdq_unpack_act(const void *act, int8_t *codes, int32_t M_pad, int32_t K, int32_t is_unsigned, void *stream);
int svdq_unpack_scales(const void *simg, void *natural, int32_t ROWS, int32_t G, void *stream);

/* ------------------------------------------------------------------------------------------
 * Launch profiler (used by bench.py for the roofline line).  While enabled, every
 * svdq_gemm_w4a4 / svdq_quantize call brackets its kernel launch with two hipEvents recorded on
 * the launch stream.  svdq_prof_read synchronises the recorded events and returns, per kernel
 * class (0 = gemm_w4a4, 1 = quantize, 2 = attention: 4*L*L*H*128 flops, 3 = gemv_awq: bytes read), the number of launches, the summed kernel time in
 * milliseconds and the summed ALGORITHMIC work (gemm: 2*M_pad*N*K + 2*M_pad*N*R operations;
 * quantize: bytes read + written).  Process-global state, guarded by a mutex; off by default.
 * ------------------------------------------------------------------------------------------ */
int svdq_prof_enable(int32_t max_launches); /* 0 disables and frees the event pool */
int svdq_prof_reset(void);
/* Restrict the bracketing to the kernel classes whose bit is set (default: all).  An event pair costs ~3 us of
 * queue serialisation per launch, so bench.py brackets only the kernel its roofline line is about. */
int svdq_prof_select(uint32_t class_mask);
int svdq_prof_read(int32_t kernel_class, int64_t *launches, double *total_ms, double *total_work);
/* Sub-classes (ABI 18): a gemm_w4a4 launch is recorded under its epilogue variant.  svdq_prof_read(0, ...) still sums every GEMM launch;
 * svdq_prof_read(SVDQ_PROF_GEMM_VARIANT(fuse), ...) returns the launches of one epilogue (SVDQ_FUSE_NONE / _SILU / _GELU_QUANT / _RMSNORM_ROPE),
 * so that a bench line can show which variant moved. */
#define SVDQ_PROF_GEMM_VARIANT(fuse) (0 | (((fuse) + 1) << 8))

/* thread-local message of the last failing call on this thread ("" if none) */
const char *svdq_last_error(void);
/* SVDQ_ABI_VERSION the library was built with */
int svdq_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVDQ_AMD_H */
