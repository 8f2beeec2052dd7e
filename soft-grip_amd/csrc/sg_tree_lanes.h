// sg_tree_lanes.h -- the tree pipeline's BULK-SYNCHRONOUS vocabulary and its two targets (part of sg_tree.h).
//
// SGT_DEVICE says which target this pass of the compiler is: the gfx950 kernel (one env per wavefront, a lane per work item) or the host
// (tests/emu, the sanitizer drivers: a parallel loop is a serial loop, a wavefront sum the identity).  Everything that differs between the
// two is named here -- the loops and barriers, the cross-lane primitives with their host twins, the address-space qualifiers, the calling
// convention of the stage functions, the profiling stamps -- so that the parts below are written once.
//
// The knock-outs (-DSGT_X_..., `build_native.py --ko NAME -DSGT_X_...`: experiment and reproducer builds, never the product).  Each puts an
// earlier or simpler version of one device path back; the host builds take the simple versions anyway:
//   SGT_X_ROWS1LANE     the free object's joint-fix rows on ONE lane (free_fix_rows' portable loop) instead of blocks over the wavefront
//   SGT_X_ROWS8LANE     ... on eight lanes, one after the other (free_fix_rows' DPP version) instead of the blocks
//   SGT_X_BLOCKED_CALL  free_fix_rows_blocked as a called function instead of inlined into the sweep
//   SGT_X_EQSYNC        the sweep's equality rounds with a barrier a round (the emulation's loop) instead of pipelined
//   SGT_X_NOLG          the chain limit rows one lane per chain instead of a lane group per chain
//   SGT_X_NOSTREAM      commuting contacts level by level, one lane per chain, instead of one stream per chain on a lane group
//   SGT_X_NOSF          serial contacts always bulk-synchronous (two barriers a contact), never the wave-synchronous pass (serial_fast)
//   SGT_X_WSSERIAL      the warmstart's a = M^-1 J' f with every word walking the contact records itself instead of lists by scalar reads
//   SGT_X_NOREGLDL      L'DL pivot by pivot through the work space instead of in registers (sg_tree_frame.inc factor_all)
//   SGT_X_MONO          every stage pasted into the kernel (r04's layout, the dropped stores of DESIGN 4.10; scripts/repro/tree_mono)
//   SGT_X_TAP           the tendon row's intermediates into spare words of S.red (scripts/repro/tree_mono, tests/emu `make dbg`)
//   (sg_math.h has SGT_X_NOQCQP)
#pragma once

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define SGT_DEVICE 1
#else
#define SGT_DEVICE 0
#endif

namespace sgt {

// section stamps (profiling build only: build_native.py --prof, scripts/tree_section_profile.py): lane 0 adds the cycles since the
// previous stamp to secprof[k]
#if defined(SG_SECTION_PROF) && defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define SGT_STAMP(k)                                                                  \
  do {                                                                                \
    if (threadIdx.x == 0) {                                                           \
      const long long t_ = clock64();                                                 \
      atomicAdd(&A.secprof[k], (unsigned long long)(t_ - sgt_t_last));                \
      sgt_t_last = t_;                                                                \
    }                                                                                 \
  } while (0)
#define SGT_STAMP_INIT() long long sgt_t_last = clock64()
#define SGT_STAMP_RESET() sgt_t_last = clock64()   /* after a called stage that kept its own stamps */
#else
#define SGT_STAMP_RESET() ((void)0)
#define SGT_STAMP(k) ((void)0)
#define SGT_STAMP_INIT() ((void)0)
#endif

// a parallel loop over the composite's elements whose per-item constants live in a small per-lane array across loops (the sweep's row
// constants: read from the work space ONCE, not once per sweep): e the element, t its slot in the lane's array (N <= 256: four a lane)
#define SGT_NSLOT (SGT_DEVICE ? 4 : 256)
#if SGT_DEVICE
#define SGT_PAR_SLOT(e, t, n) _Pragma("unroll") for (int t = 0, e = (int)threadIdx.x; t < 4; t++, e += 64) if (e < (n))
#elif defined(SGT_EMU_REVERSE)
#define SGT_PAR_SLOT(e, t, n) for (int e = (n) - 1, t = e; e >= 0; e--, t = e)
#else
#define SGT_PAR_SLOT(e, t, n) for (int e = 0, t = 0; e < (n); e++, t = e)
#endif
#if SGT_DEVICE
#define SGT_FIRST ((int)threadIdx.x)
#define SGT_STRIDE 64
#define SGT_PAR(i, n) for (int i = (int)threadIdx.x; i < (n); i += 64)
#define SGT_ONE if (threadIdx.x == 0)
#if defined(SGT_X_ROWS1LANE)
#define SGT_ROW_LANES if (threadIdx.x == 0)
#else
#define SGT_ROW_LANES if (threadIdx.x < 8)   // free_fix_rows: the free body's serial joint-fix rows on eight lanes
#endif
#define SGT_SYNC() __syncthreads()
// cross-lane moves without LDS: DPP on the two halves of a double (row_ror:n = 0x120 + n, rotation inside a row of 16 lanes)
template <int CTRL>
__device__ __forceinline__ double dpp64(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// sum over the 16 lanes of a row (a LANE GROUP: one finger chain's lanes in the sweep), result in all 16: a butterfly of rotations
__device__ __forceinline__ double rowsum16(double x) {
  x += dpp64<0x128>(x);
  x += dpp64<0x124>(x);
  x += dpp64<0x122>(x);
  x += dpp64<0x121>(x);
  return x;
}
__device__ __forceinline__ double readlane64(double x, int l) {   // l uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
// sum over the wavefront, result in all lanes: the rows by rotations, the four rows by scalar reads (was six ds_bpermute round trips)
__device__ __forceinline__ double wsum(double x) {
  x = rowsum16(x);
  return ((readlane64(x, 0) + readlane64(x, 16)) + readlane64(x, 32)) + readlane64(x, 48);
}
__device__ __forceinline__ double wmax(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ int lds_inc(int* p) { return atomicAdd(p, 1); }
#else
#define SGT_FIRST 0
#define SGT_STRIDE 1
#if defined(SGT_EMU_REVERSE)
// host emulation, order-checking build (tests/emu `make rev`): every parallel loop runs its items in DESCENDING order.  A parallel loop's
// items must not depend on one another (on the device they run in lockstep, 64 at a time); the ascending serial loop of the normal
// emulation satisfies any dependency of item i on an item j < i by accident.  Same results in both orders = no such dependency.
#define SGT_PAR(i, n) for (int i = (n) - 1; i >= 0; i--)
#else
#define SGT_PAR(i, n) for (int i = 0; i < (n); i++)
#endif
#define SGT_ONE if (true)
#define SGT_ROW_LANES if (true)
#define SGT_SYNC() ((void)0)
inline double wsum(double x) { return x; }
inline double wmax(double x) { return x; }
inline int lds_inc(int* p) { return (*p)++; }
#endif

#if defined(__HIPCC__)
#define SGT_NOINLINE __host__ __device__ __attribute__((noinline))
#else
#define SGT_NOINLINE __attribute__((noinline))
#endif
// pointers into the env's LDS block, typed as such for an out-of-line function: through generic pointers the loads are FLAT, whose
// completion the compiler can only wait for all at once -- which turns a prefetch into a stall
#if SGT_DEVICE
#define SGT_LDSP __attribute__((address_space(3)))
#define SGT_CONST __attribute__((address_space(4)))
#define SGT_GLOBP __attribute__((address_space(1)))
#else
#define SGT_LDSP
#define SGT_CONST
#define SGT_GLOBP
#endif

// ---------------------------------------------------------------- the step's stages, each a function of its own
// One env's whole step used to be ONE function: every stage below pasted into the kernel, ~60 array pointers, the plan's tables and
// every stage's temporaries competing for one register allocation -- 850 scalar and 550 - 1 650 vector registers spilled (r04
// profile), the scalar ones into lanes of vector registers that were themselves parked in accumulation registers.  Builds of that
// function that differed only in unrelated places (a profiling stamp, a debugging copy at the end) then disagreed about single
// stores of the contact rows' build -- a word of a contact's record keeping its old value -- which is how a fuzz scene went
// to NaN on one build and not on the next.  Now: the step is a sequence of CALLED functions, one per group of
// stages, each with its own registers; what they hand each other lives in the env's LDS block and work space anyway, and the
// step's few scalars (flags, counts, the touch bits) travel in S.ctx.  On the device a stage finds the launch arguments in the
// kernel-argument segment (uniform: scalar loads) and its env in the workgroup id; on the host they are passed.
#if SGT_DEVICE
#define SGT_STAGE_PARAMS SGT_LDSP double* lds_
#define SGT_STAGE_CALL(NAME) tree_stage_##NAME<CHD>((SGT_LDSP double*)lds_base)
#else
#define SGT_STAGE_PARAMS const TreeArgs& A, const int env, double* lds_base
#define SGT_STAGE_CALL(NAME) tree_stage_##NAME<CHD>(A, env, lds_base)
#endif
// the stages (sg_tree_stage_*.h):
// dynamics:    checks, kinematics, tendons, mass matrix, L'DL + M^-1, bias and smooth accelerations (chains, sliders, free object)
// collision:   block culling, the pair walks, rank, narrowphase
// constraints: constraint rows (equality, limits, contacts), warmstart, the PGS sweeps (tree_sweep)
// finish:      qacc, sensors, Euler with implicit damping
// (SGT_X_MONO: the r04 layout that produced the dropped stores -- every stage pasted into the kernel, one register allocation for the
//  whole step -- kept buildable for scripts/repro/tree_mono: `build_native.py --ko mono -DSGT_X_MONO`; never the product)
#if defined(SGT_X_MONO) && defined(__HIPCC__)
#define SGT_STAGE_ATTR __host__ __device__ __forceinline__
#else
#define SGT_STAGE_ATTR SGT_NOINLINE
#endif

}  // namespace sgt
