// Wide ray cast for gfx950 (MI355X): both ray casts in one persistent launch over a 4-WIDE collapse of the binary SBVH, one 128-byte
// record -- one memory-side line -- per dependent step (GMUPT_TRAVERSAL=wide).
//
// Why the walk may be restructured at all.  The reference never prunes a box against the current hit: a child is visited iff its slab
// test returns > 0 (extensionRayCast.hlsl:79-94,132-159).  So the set of leaves a ray reaches is fixed -- every leaf whose box and all of
// whose ancestors' boxes are hit -- and so are the triangle tests.  A child's box lies inside its parent's box and the slab arithmetic
// is monotone in the plane coordinates (binary32 subtraction and multiplication by the same 1 / d are monotone; NaN-dropping min / max
// keep the child's interval inside the parent's), so "child hit" implies "parent hit" and testing only SOME of a leaf's ancestors
// reaches exactly the same leaves.  Two conditions, both checked on the host when the collapse is built (gmupt_capi.hip):
//   - every child box lies inside its parent's box (a tree that violates it is walked by the binary kernel);
//   - the one case where monotonicity fails: a ray with an infinite 1 / d component (d = 0 on an axis; the reference's 8-bit random
//     numbers make 0.3 % of the bounces off axis-aligned walls such rays) whose origin lies exactly in the plane of a box that is FLAT
//     on that axis.  0 x inf = NaN is dropped by min / max, so the flat box imposes no condition, while a non-flat parent that has
//     this plane as a FACE is missed (near = far = +-inf).  An inner node with a child that is flat on one of its faces is therefore
//     never opened by the collapse: its own box test is kept, exactly where the reference makes it.
// What the visit ORDER decides is only which of two accepted hits with bitwise equal t wins (`t < distance` is strict,
// extensionRayCast.hlsl:64-74).  This kernel walks in whatever order is cheapest, notices when the closest hit of an extension ray is
// such a tie between two DIFFERENT triangles (the duplicated references of one triangle give identical hit records either way) and
// then PARKS the ray in its lane; parked rays are walked again in the reference's binary near-first order on the packed binary copy
// (Node64), all parked lanes of the wave at once -- at the end of the wave's life, or as soon as a quarter of its lanes are parked.
// A handful of rays per launch on ordinary scenes, most rays on the adversarial grid meshes of the tests.  A shadow ray is any-hit:
// its result does not depend on the order at all (shadowRayCast.hlsl:88-91).
//
// Per lane: ONE array of kWideStack words in LDS ([entry][lane], conflict-free) holds two stacks growing towards each other -- inner
// nodes still to visit from the bottom up, leaves still to test from the top down.  A step fetches one WNode (seven 16-byte pieces:
// six planes x four slots, four links), does the four slab tests, keeps one hit inner slot as the next node and pushes the other
// hits.  Leaves are tested in wave-wide bursts, one triangle record per step, fetched together with the node of the walking lanes
// (everything around the walk is pt_cast_plumbing.hpp).  A lane whose inner stack alone fills its LDS share gives the wide walk of that ray up and parks it as well (the exact
// walk has a bounds-checked global overflow).  Drain: finished lanes take the BOTTOM inner entry of busy lanes (the largest subtree
// left) and report their best hit back; results merge by "smaller t wins, equal t is a tie".
//
// The pushes of a step are branch-free: for the four slots in turn `sl[pa] = link; pa += (hit and inner)`, then for the four slots in
// turn `sl[pb] = link; pb -= (hit and leaf)` -- eight unconditional LDS stores, each at the current top, the top advanced by the
// predicate.  The next node is the LAST hit inner slot, taken from its register (the visit order is free, see above); its copy is the
// entry on top of the inner stack, so `pa--` drops it and it is never read back.  Why no store destroys a live entry (pa0, pb0: the
// tops before the step; cI, cL: inner and leaf hits of the step, cI + cL <= 4):
//   - a lane steps only with pb0 - pa0 >= kWideRoom - 1 = 3: the slots pa0 .. pb0, at least four, are free, and every store of the step
//     lands in pa0 .. pa0 + 3 or pb0 - 3 .. pb0, inside them (and inside the lane's LDS share);
//   - the inner stores run first.  One that does not advance leaves garbage at the top, which is free: the next advancing store
//     overwrites it, and at worst it is slot pa0 + 3 == pb0, which a later real leaf store overwrites or which stays free;
//   - after the step the live inner entries end at pa0 + cI - 2 (the one at pa0 + cI - 1 is in the register, its copy is dead);
//   - a leaf store that does not advance writes at pb0 - s, s <= cL leaf hits before it.  It would reach a live inner entry only with
//     pb0 - cL <= pa0 + cI - 2, i.e. pb0 - pa0 <= cI + cL - 2 <= 2: not with the room a step requires.  Nor does it reach a live leaf
//     entry: those are above pb0, or at pb0 - k, k < s, written earlier in this step;
//   - an empty slot (NaN planes, link kDone) never hits, so it never advances; with no inner hit the pop reads sl[pa0 - 1], which no
//     store of the step touches; the hand-over to a helper reads sl[bottom], live and below pa0; the reset of an occluded shadow ray
//     (pa = bottom, pb = S - 1) declares everything dead.
// The argument uses the room condition only, not kWideStack: it holds for the 8-word test build as for the shipped 24 words.
#include "pt_cast_plumbing.hpp"
#include "pt_travtables.hpp"
#include "pt_launch.hpp"

namespace gmupt {

#ifndef GMUPT_WIDE_STACK
#define GMUPT_WIDE_STACK 24
#endif
#ifndef GMUPT_WIDE_TOP
#define GMUPT_WIDE_TOP 512
#endif
#ifndef GMUPT_WIDE_REPS
#define GMUPT_WIDE_REPS 6
#endif
#ifndef GMUPT_WIDE_PARK
#define GMUPT_WIDE_PARK 16
#endif
constexpr int kWideStack = GMUPT_WIDE_STACK;   // LDS words per lane shared by the two stacks
constexpr int kWideTop = GMUPT_WIDE_TOP;       // WNodes of the tree top kept in LDS
constexpr int kWideRoom = 4;                   // a node step pushes at most four entries
constexpr int kWidePark = GMUPT_WIDE_PARK;     // parked lanes of a wave that trigger the exact walk before the wave has run dry
static_assert(kWideStack * kDefBlock * 4 + kWideTop * 128 <= 160 * 1024, "LDS of one CU (wide layout)");
constexpr int kWideOvf = kMaxStack + 2 > kWideStack ? kMaxStack + 2 - kWideStack : 0;   // the exact walk's stack: the lane's LDS share, then this many entries of the global overflow buffer

typedef int vec4i __attribute__((ext_vector_type(4)));

// One WNode into registers: from the LDS copy of the tree top (the top walk), or from global memory (everything below the top).
// The planes of a WNode in RAY-SIGN order: q0 .. q2 = the plane of each axis the ray meets first (row `axis` for a positive, row 5 - axis for a
// negative 1 / d), q3 .. q5 = the other one.  Which row is a per-lane byte offset (RayPk's packed `sg`: bytes 0..2 = 0|80, 16|64, 32|48), added to
// the lane's record address with one SDWA add per axis; the far row of every axis is at (2 * record + 80) - near address.
__device__ __forceinline__ uint32_t add_byte0(uint32_t a, uint32_t b) { uint32_t r; asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ uint32_t add_byte1(uint32_t a, uint32_t b) { uint32_t r; asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ uint32_t add_byte2(uint32_t a, uint32_t b) { uint32_t r; asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(a), "v"(b)); return r; }
struct PlaneAddr { uint32_t nx, ny, nz, fx, fy, fz, rec; };
__device__ __forceinline__ PlaneAddr plane_addresses(int cur, uint32_t sg)
{
    PlaneAddr a; a.rec = (uint32_t)cur * 128u;
    const uint32_t k2 = a.rec * 2u + 80u;
    a.nx = add_byte0(a.rec, sg); a.ny = add_byte1(a.rec, sg); a.nz = add_byte2(a.rec, sg);
    a.fx = k2 - a.nx; a.fy = k2 - a.ny; a.fz = k2 - a.nz;
    return a;
}
__device__ __forceinline__ void load_wnode_lds_signed(const float4* s_top, const PlaneAddr a, vec4f& q0, vec4f& q1, vec4f& q2, vec4f& q3, vec4f& q4, vec4f& q5, vec4i& lk)
{
    const uint32_t base = (uint32_t)(uintptr_t)((const GMUPT_AS_LDS vec4f*)(s_top));     // 0: the top is the first thing in LDS
    q0 = *(const GMUPT_AS_LDS vec4f*)(uintptr_t)(base + a.nx); q1 = *(const GMUPT_AS_LDS vec4f*)(uintptr_t)(base + a.ny); q2 = *(const GMUPT_AS_LDS vec4f*)(uintptr_t)(base + a.nz);
    q3 = *(const GMUPT_AS_LDS vec4f*)(uintptr_t)(base + a.fx); q4 = *(const GMUPT_AS_LDS vec4f*)(uintptr_t)(base + a.fy); q5 = *(const GMUPT_AS_LDS vec4f*)(uintptr_t)(base + a.fz);
    lk = *(const GMUPT_AS_LDS vec4i*)(uintptr_t)(base + a.rec + 96u);
}
__device__ __forceinline__ void load_wnode_glb_signed(__amdgpu_buffer_rsrc_t nodes, const PlaneAddr a, vec4f& q0, vec4f& q1, vec4f& q2, vec4f& q3, vec4f& q4, vec4f& q5, vec4i& lk)
{
    q0 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(nodes, (int)a.nx, 0, 0));
    q1 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(nodes, (int)a.ny, 0, 0));
    q2 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(nodes, (int)a.nz, 0, 0));
    q3 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(nodes, (int)a.fx, 0, 0));
    q4 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(nodes, (int)a.fy, 0, 0));
    q5 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(nodes, (int)a.fz, 0, 0));
    lk = __builtin_bit_cast(vec4i, __builtin_amdgcn_raw_buffer_load_b128(nodes, (int)a.rec + 96, 0, 0));
}

// source-triangle number of a reference (word 10 of its Tri48 record): equal for the duplicated references of one triangle
__device__ __forceinline__ uint32_t tri_canon(__amdgpu_buffer_rsrc_t tris, int i)
{
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(tris, i * 48 + 40, 0, 0);
}

// Packed binary32 arithmetic (v_pk_add_f32 / v_pk_mul_f32: the same IEEE operations as the scalar instructions, two at a time) as the
// machine instructions themselves.  Why not vector types and the compiler: (1) it puts a canonicalising `v_max x, x` in front of every
// fminf / fmaxf that consumes a packed product; (2) a scalar operand that both halves must see (a ray component) it either copies into
// a register pair of its own -- 18 registers this kernel does not have -- or re-aligns through SCRATCH memory in every step; the
// instruction itself can take either half of an aligned pair for both results (op_sel).  So the ray lives in five aligned pairs (RayPk)
// and each instruction names the half it broadcasts (op_sel).  Every statement of packed instructions ends with `s_nop 0`: on gfx950 a
// packed result may not be read by the very next instruction (the compiler pads its own packed code the same way; it cannot see into an
// asm statement), and inside a statement no instruction reads the result of the one before it.
// v_min / v_max / v_min3 / v_max3 return the non-NaN operand like the HLSL min / max, and no operand here can be a signalling NaN
// (products, and the quiet NaNs of empty slots).
__device__ __forceinline__ float v_min(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float v_max(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float v_min3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float v_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// The lane's ray in five aligned register pairs: (o.x, o.y), (o.z, 1/d.z), (1/d.x, 1/d.y), (d.x, d.y), (d.z, sg).  sg (raw bits): byte k = the byte
// offset of the plane row the ray meets first on axis k (load_wnode_*_signed), byte 3 = 1 when a component of 1 / d is infinite or NaN
// (a direction component that is zero, denormal or NaN): for such a ray (plane - o) * (1 / d) can be NaN, and min / max decide which plane
// is the near one -- the wave then takes the general form of the test.
struct RayPk { vec2f oxy, ozi, ixy, dxy, dzz; };
__device__ __forceinline__ uint32_t ray_sg(const RayPk& r) { return __builtin_bit_cast(vec2u, r.dzz).y; }
__device__ __forceinline__ f3 ray_o(const RayPk& r) { return mk3(r.oxy.x, r.oxy.y, r.ozi.x); }
__device__ __forceinline__ f3 ray_inv(const RayPk& r) { return mk3(r.ixy.x, r.ixy.y, r.ozi.y); }
__device__ __forceinline__ f3 ray_d(const RayPk& r) { return mk3(r.dxy.x, r.dxy.y, r.dzz.x); }
__device__ __forceinline__ void ray_set(RayPk& r, f3 o, f3 d)
{
    r.oxy.x = o.x; r.oxy.y = o.y; r.ozi.x = o.z; r.ixy.x = 1.0f / d.x; r.ixy.y = 1.0f / d.y; r.ozi.y = 1.0f / d.z;
    r.dxy.x = d.x; r.dxy.y = d.y; r.dzz.x = d.z;
    const vec2u ib = __builtin_bit_cast(vec2u, r.ixy), zb = __builtin_bit_cast(vec2u, r.ozi);      // (whole-vector casts: a bit cast of a vector ELEMENT reads element 0)
    const uint32_t bx = ib.x, by = ib.y, bz = zb.y;
    const bool special = ((bx & 0x7F800000u) == 0x7F800000u) | ((by & 0x7F800000u) == 0x7F800000u) | ((bz & 0x7F800000u) == 0x7F800000u);
    const uint32_t sg = ((bx >> 31) ? 80u : 0u) | ((by >> 31) ? (64u << 8) : (16u << 8)) | ((bz >> 31) ? (48u << 16) : (32u << 16)) | (special ? (1u << 24) : 0u);
    vec2u dz = __builtin_bit_cast(vec2u, r.dzz); dz.y = sg; r.dzz = __builtin_bit_cast(vec2f, dz);
}

#define GMUPT_LO(Q) __builtin_shufflevector(Q, Q, 0, 1)
#define GMUPT_HI(Q) __builtin_shufflevector(Q, Q, 2, 3)
// the min / max tree of ray_box (extensionRayCast.hlsl:79-94) on one slot; "hit" is `result > 0`, i.e. t1 >= t0 and (t0 > 0 ? t0 : t1) > 0,
// which is t1 >= t0 && t1 > 0 (t1 >= t0 > 0 implies t1 > 0; a NaN fails both forms)
__device__ __forceinline__ bool slab_hit_pk(float nx, float ny, float nz, float fx, float fy, float fz)
{
    const float t1 = v_min3(v_max(fx, nx), v_max(fy, ny), v_max(fz, nz));
    const float t0 = v_max3(v_min(fx, nx), v_min(fy, ny), v_min(fz, nz));
    return (t1 >= t0) & (t1 > 0.0f);
}
// the same test when the near / far plane of every axis is known (rows in ray-sign order, 1 / d finite): (near - o) / d <= (far - o) / d by the
// monotonicity of the two rounded operations, so min(f, n) IS n and max(f, n) IS f -- six of the eight min / max of a slot go
__device__ __forceinline__ bool slab_hit_ordered(float nx, float ny, float nz, float fx, float fy, float fz)
{
    const float t1 = v_min3(fx, fy, fz);
    const float t0 = v_max3(nx, ny, nz);
    return (t1 >= t0) & (t1 > 0.0f);
}
// the four slab tests of a step: (plane - o) * (1 / d) for two slots per packed instruction, then the min / max tree of ray_box per slot
// (GENERAL: wave-uniform; the rows may be in either order for it)
__device__ __forceinline__ void slab_hits4(const vec4f q0, const vec4f q1, const vec4f q2, const vec4f q3, const vec4f q4, const vec4f q5, const RayPk& ray,
                                           bool& h0, bool& h1, bool& h2, bool& h3, const bool general = true)
{
    // (plane - o) * (1 / d), one plane row (four slots) per statement: two subtractions, two multiplications -- a product is read two
    // instructions after its difference was written, so one wait state at the end covers the statement
    vec2f nxa, nxb, nya, nyb, nza, nzb, fxa, fxb, fya, fyb, fza, fzb;
#define GMUPT_ROW(A, B, Q, O, OSEL, INV, ISEL) \
    asm("v_pk_add_f32 %0, %2, %4 " OSEL " neg_lo:[0,1] neg_hi:[0,1]\n\tv_pk_add_f32 %1, %3, %4 " OSEL " neg_lo:[0,1] neg_hi:[0,1]\n\t" \
        "v_pk_mul_f32 %0, %0, %5 " ISEL "\n\tv_pk_mul_f32 %1, %1, %5 " ISEL "\n\ts_nop 0" \
        : "=&v"(A), "=&v"(B) : "v"(GMUPT_LO(Q)), "v"(GMUPT_HI(Q)), "v"(O), "v"(INV))
    GMUPT_ROW(nxa, nxb, q0, ray.oxy, "op_sel_hi:[1,0]", ray.ixy, "op_sel_hi:[1,0]");
    GMUPT_ROW(nya, nyb, q1, ray.oxy, "op_sel:[0,1]", ray.ixy, "op_sel:[0,1]");
    GMUPT_ROW(nza, nzb, q2, ray.ozi, "op_sel_hi:[1,0]", ray.ozi, "op_sel:[0,1]");
    GMUPT_ROW(fxa, fxb, q3, ray.oxy, "op_sel_hi:[1,0]", ray.ixy, "op_sel_hi:[1,0]");
    GMUPT_ROW(fya, fyb, q4, ray.oxy, "op_sel:[0,1]", ray.ixy, "op_sel:[0,1]");
    GMUPT_ROW(fza, fzb, q5, ray.ozi, "op_sel_hi:[1,0]", ray.ozi, "op_sel:[0,1]");
#undef GMUPT_ROW
    if (general) {
        h0 = slab_hit_pk(nxa.x, nya.x, nza.x, fxa.x, fya.x, fza.x); h1 = slab_hit_pk(nxa.y, nya.y, nza.y, fxa.y, fya.y, fza.y);
        h2 = slab_hit_pk(nxb.x, nyb.x, nzb.x, fxb.x, fyb.x, fzb.x); h3 = slab_hit_pk(nxb.y, nyb.y, nzb.y, fxb.y, fyb.y, fzb.y);
    } else {
        h0 = slab_hit_ordered(nxa.x, nya.x, nza.x, fxa.x, fya.x, fza.x); h1 = slab_hit_ordered(nxa.y, nya.y, nza.y, fxa.y, fya.y, fza.y);
        h2 = slab_hit_ordered(nxb.x, nyb.x, nzb.x, fxb.x, fyb.x, fzb.x); h3 = slab_hit_ordered(nxb.y, nyb.y, nzb.y, fxb.y, fyb.y, fzb.y);
    }
}

// Moeller-Trumbore (extensionRayCast.hlsl:38-62 == shadowRayCast.hlsl:16-40) on the TWO triangles of a TriPair at once: every operation of
// tri_compute_flat, in its order, on a (first, second) pair of operands -- packed where the machine has the instruction (sub, mul, add),
// the scalar instruction twice where it has not (the correctly rounded division, the comparisons).  okA / okB: not rejected.
struct PairHit { vec2f t, u, v; bool okA, okB; bool last; };
__device__ __forceinline__ PairHit tri_pair_compute(const vec4f a0, const vec4f a1, const vec4f a2, const vec4f a3, const vec4f a4, const RayPk& ray)
{
    const vec2f v0x = GMUPT_LO(a0), v0y = GMUPT_HI(a0), v0z = GMUPT_LO(a1), e1x = GMUPT_HI(a1), e1y = GMUPT_LO(a2), e1z = GMUPT_HI(a2);
    const vec2f e2x = GMUPT_LO(a3), e2y = GMUPT_HI(a3), e2z = GMUPT_LO(a4);
    PairHit h;
    // the operations of tri_compute_flat (pt_traverse_common.hpp), in its order, in four statements of independent instructions (one
    // wait state per statement: no result is read by the instruction that follows the one that wrote it)
    vec2f px, py, pz, tx, ty, tz, m1, m2, m3;
    asm("v_pk_mul_f32 %0, %11, %15 op_sel:[0,1]\n\t"                                    // pvec = cross3(d, e2): e2z d.y
        "v_pk_mul_f32 %6, %10, %16 op_sel_hi:[1,0]\n\t"                                 //   e2y d.z
        "v_pk_mul_f32 %1, %9, %16 op_sel_hi:[1,0]\n\t"                                  //   e2x d.z
        "v_pk_mul_f32 %7, %11, %15 op_sel_hi:[1,0]\n\t"                                 //   e2z d.x
        "v_pk_mul_f32 %2, %10, %15 op_sel_hi:[1,0]\n\t"                                 //   e2y d.x
        "v_pk_mul_f32 %8, %9, %15 op_sel:[0,1]\n\t"                                     //   e2x d.y
        "v_pk_add_f32 %3, %17, %12 op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"       // tvec = o - v0
        "v_pk_add_f32 %4, %17, %13 op_sel:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %5, %18, %14 op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %0, %0, %6 neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %1, %1, %7 neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %2, %2, %8 neg_lo:[0,1] neg_hi:[0,1]\n\ts_nop 0"
        : "=&v"(px), "=&v"(py), "=&v"(pz), "=&v"(tx), "=&v"(ty), "=&v"(tz), "=&v"(m1), "=&v"(m2), "=&v"(m3)
        : "v"(e2x), "v"(e2y), "v"(e2z), "v"(v0x), "v"(v0y), "v"(v0z), "v"(ray.dxy), "v"(ray.dzz), "v"(ray.oxy), "v"(ray.ozi));
    vec2f det, uu, c1, c2, c3, c4;
    asm("v_pk_mul_f32 %0, %6, %9\n\tv_pk_mul_f32 %2, %7, %10\n\tv_pk_mul_f32 %3, %8, %11\n\t"        // dot3(e1, pvec)
        "v_pk_mul_f32 %1, %12, %9\n\tv_pk_mul_f32 %4, %13, %10\n\tv_pk_mul_f32 %5, %14, %11\n\t"     // dot3(tvec, pvec)
        "v_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %1, %1, %4\n\tv_pk_add_f32 %0, %0, %3\n\tv_pk_add_f32 %1, %1, %5\n\ts_nop 0"
        : "=&v"(det), "=&v"(uu), "=&v"(c1), "=&v"(c2), "=&v"(c3), "=&v"(c4)
        : "v"(e1x), "v"(e1y), "v"(e1z), "v"(px), "v"(py), "v"(pz), "v"(tx), "v"(ty), "v"(tz));
    vec2f qx, qy, qz;
    asm("v_pk_mul_f32 %0, %7, %11\n\tv_pk_mul_f32 %3, %8, %10\n\tv_pk_mul_f32 %1, %8, %9\n\t"        // qvec = cross3(tvec, e1)
        "v_pk_mul_f32 %4, %6, %11\n\tv_pk_mul_f32 %2, %6, %10\n\tv_pk_mul_f32 %5, %7, %9\n\t"
        "v_pk_add_f32 %0, %0, %3 neg_lo:[0,1] neg_hi:[0,1]\n\tv_pk_add_f32 %1, %1, %4 neg_lo:[0,1] neg_hi:[0,1]\n\tv_pk_add_f32 %2, %2, %5 neg_lo:[0,1] neg_hi:[0,1]\n\ts_nop 0"
        : "=&v"(qx), "=&v"(qy), "=&v"(qz), "=&v"(m1), "=&v"(m2), "=&v"(m3)
        : "v"(tx), "v"(ty), "v"(tz), "v"(e1x), "v"(e1y), "v"(e1z));
    vec2f invDet; invDet.x = 1.0f / det.x; invDet.y = 1.0f / det.y;
    vec2f vv, tt;
    asm("v_pk_mul_f32 %1, %7, %10 op_sel_hi:[1,0]\n\tv_pk_mul_f32 %3, %8, %10 op_sel:[0,1]\n\tv_pk_mul_f32 %4, %9, %11 op_sel_hi:[1,0]\n\t"   // dot3(d, qvec)
        "v_pk_mul_f32 %2, %12, %7\n\tv_pk_mul_f32 %5, %13, %8\n\tv_pk_mul_f32 %6, %14, %9\n\t"                                                // dot3(e2, qvec)
        "v_pk_mul_f32 %0, %0, %15\n\t"                                                                                                          // u
        "v_pk_add_f32 %1, %1, %3\n\tv_pk_add_f32 %2, %2, %5\n\tv_pk_add_f32 %1, %1, %4\n\tv_pk_add_f32 %2, %2, %6\n\t"
        "v_pk_mul_f32 %1, %1, %15\n\tv_pk_mul_f32 %2, %2, %15\n\ts_nop 0"                                                                      // v, t
        : "+v"(uu), "=&v"(vv), "=&v"(tt), "=&v"(c1), "=&v"(c2), "=&v"(c3), "=&v"(c4)
        : "v"(qx), "v"(qy), "v"(qz), "v"(ray.dxy), "v"(ray.dzz), "v"(e2x), "v"(e2y), "v"(e2z), "v"(invDet));
    h.u = uu; h.v = vv; h.t = tt;
    h.okA = !((det.x > -kEpsilon && det.x < kEpsilon) | (h.u.x < 0.0f) | (h.u.x > 1.0f) | (h.v.x < 0.0f) | (h.u.x + h.v.x > 1.0f));
    h.okB = !((det.y > -kEpsilon && det.y < kEpsilon) | (h.u.y < 0.0f) | (h.u.y > 1.0f) | (h.v.y < 0.0f) | (h.u.y + h.v.y > 1.0f));
    h.last = __builtin_bit_cast(vec4u, a4).z != 0u;   // (whole-vector bit cast: __builtin_bit_cast of a vector ELEMENT reads element 0 with this compiler)
    return h;
}
#undef GMUPT_LO
#undef GMUPT_HI

// ---- where the rays come from and where the results go: a compile-time policy of k_cast_w.
// StateIO is the path tracer's own ray cast (queues and path state of the renderer, extensionRayCast.hlsl / shadowRayCast.hlsl); QueryIO
// serves gmupt_trace_rays: caller arrays of gmupt_ray in, gmupt_hit records and occluded flags out.  Everything else -- the walk, the
// parking, the exact walk, the watchdog -- is the same code; the work counters and the statistics are whatever p.travCounters and p.stats
// point to (the query launcher gives it buffers of its own).  The ray is read by path-state field (ray3 / rayf): the StateIO instantiations
// then compile to the instruction stream of the kernel before the policy existed (tools/isa_compare.py).
struct StateIO {
    using Params = RenderParams;
    __device__ static __forceinline__ void prologue(const Params& p) { shadow_counter_epilogue(p); }
    __device__ static __forceinline__ uint32_t count(const Params& p, int phase) { return phase == 0 ? p.qc[QC_EXT_COUNT] : p.qc[QC_SHADOWRAY]; }  // extensionRayCast.hlsl:205, shadowRayCast.hlsl:151
    __device__ static __forceinline__ const uint32_t* queue(const Params& p, int phase) { return p.queues + (size_t)(phase == 0 ? Q_EXT_RAY : Q_SHADOW_RAY) * p.P; }
    __device__ static __forceinline__ uint32_t entry(const uint32_t* q, uint32_t i) { return q[i]; }
    __device__ static __forceinline__ f3 ray3(const Params& p, uint32_t f, uint32_t i) { return ld3(p, f, i); }
    __device__ static __forceinline__ float rayf(const Params& p, uint32_t f, uint32_t i) { return ldf(p, f, i); }
    __device__ static __forceinline__ float closest_limit(const Params&, uint32_t) { return kFltMax; }          // an extension ray has no limit
    __device__ static __forceinline__ void finish_closest(const Params& p, uint32_t index, f3 o, f3 d, float distance, float hu, float hv, int ref)
    {
        finish_extension_ray(p, index, o, d, distance, hu, hv, ref);                                            // extensionRayCast.hlsl:218-232
    }
    __device__ static __forceinline__ void finish_any(const Params& p, uint32_t index, uint32_t occluded) { stu(p, F_IN_SHADOW, index, occluded); }   // shadowRayCast.hlsl:167
};

struct QueryParams : RenderParams {
    const gmupt_ray* rays[2];   // phase 0: closest-hit rays, phase 1: any-hit rays
    uint32_t count[2];
    gmupt_hit* hits;            // one per closest-hit ray
    uint32_t* occluded;         // one per any-hit ray
    uint32_t lightCount;        // light spheres tested after the triangles (clamped to GMUPT_MAX_LIGHTS)
};

struct QueryIO {
    using Params = QueryParams;
    __device__ static __forceinline__ void prologue(const Params&) {}                                            // the renderer's counters stay as they are
    __device__ static __forceinline__ uint32_t count(const Params& p, int phase) { return p.count[phase]; }
    __device__ static __forceinline__ const uint32_t* queue(const Params&, int) { return nullptr; }
    __device__ static __forceinline__ uint32_t entry(const uint32_t*, uint32_t i) { return i; }                // identity queues, no holes
    // the path-state fields of the two ray kinds on the caller's 32-byte records (f is a constant after inlining): origin, direction, and
    // tmax as the limit of BOTH kinds (the light distance of an any-hit ray, the starting distance of a closest-hit ray)
    __device__ static __forceinline__ f3 ray3(const Params& p, uint32_t f, uint32_t i)
    {
        const float4 a = reinterpret_cast<const float4*>(p.rays[(f == F_SH_OX || f == F_SH_DX) ? 1 : 0] + i)[(f == F_RAY_DX || f == F_SH_DX) ? 1 : 0];
        return mk3(a.x, a.y, a.z);
    }
    __device__ static __forceinline__ float rayf(const Params& p, uint32_t, uint32_t i) { return p.rays[1][i].tmax; }   // F_LIGHT_DIST
    __device__ static __forceinline__ float closest_limit(const Params& p, uint32_t i) { return p.rays[0][i].tmax; }
    __device__ static __forceinline__ void finish_closest(const Params& p, uint32_t index, f3 o, f3 d, float distance, float hu, float hv, int ref)
    {
        const bool hit = ref >= 0;
        const uint32_t material = hit ? p.scene.tris[ref].materialID : 0u;
        GMUPT_LIGHT_SPHERES(p.scene.lights, p.lightCount, o, d, distance, light)                // extensionRayCast.hlsl:168-194
        float4* h = reinterpret_cast<float4*>(p.hits + index);
        // the triangle as its first reference with the same record (word 10 of Tri48): duplicated references of one triangle tie, and which
        // of them a walk meets first depends on the lanes; the lowest index is the same answer every time
        const int tri = hit ? (int)__builtin_bit_cast(uint32_t, p.trav.tris[ref].r2[2]) : -1;
        h[0] = make_float4(distance, hit ? hu : 0.0f, hit ? hv : 0.0f, __builtin_bit_cast(float, tri));
        h[1] = make_float4(__builtin_bit_cast(float, light), __builtin_bit_cast(float, material), 0.0f, 0.0f);
    }
    __device__ static __forceinline__ void finish_any(const Params& p, uint32_t index, uint32_t occluded) { p.occluded[index] = occluded; }
};

template <bool STATS, int REPS, class IO>
__global__ __launch_bounds__(kDefBlock) void k_cast_w(typename IO::Params p)
{
    constexpr int S = kWideStack;
    // one LDS object, the tree top first: a top node's LDS address is then its byte offset in the node table (cur * 128), and the plane
    // addresses of a step (load_wnode_*_signed) serve the LDS and the vector-memory fetch alike
    __shared__ float4 s_lds[kWideTop * 8 + S * kDefBlock / 4];
    float4* s_top = s_lds;
    int* s_stack = reinterpret_cast<int*>(s_lds + kWideTop * 8);
    {
        const float4* src = reinterpret_cast<const float4*>(p.trav.wnodes);
        for (uint32_t k = threadIdx.x; k < p.trav.wideTopCount * 8u; k += kDefBlock) s_top[k] = src[k];
        __syncthreads();
    }
    IO::prologue(p);
    int* sl = s_stack + threadIdx.x;     // entry i of this lane: sl[i * kDefBlock]
    TravCount tcE = { 0, 0, 0 }, tcS = { 0, 0, 0 }; uint32_t raysE = 0, raysS = 0, wInE = 0, wTrE = 0, wInS = 0, wTrS = 0;
    const TravScene& ts = p.trav;
    const uint32_t countExt = IO::count(p, 0), countSh = IO::count(p, 1);
    const uint32_t* qExt = IO::queue(p, 0);
    const uint32_t* qSh = IO::queue(p, 1);
    const __amdgpu_buffer_rsrc_t rNodes = make_rsrc(ts.wnodes, ts.wideCount * 128u);
    const __amdgpu_buffer_rsrc_t rTris = make_rsrc(ts.tris, (p.scene.numTris + 1u) * 48u);    // + the sentinel record (the exact walk; the source-triangle numbers)
    const __amdgpu_buffer_rsrc_t rPairs = make_rsrc(ts.pairs, ts.numPairs * 80u);
    const uint32_t topCount = ts.wideTopCount;
    GMUPT_CHUNK_CURSOR            // the current chunk of queue entries
    int phase = 0;
    uint32_t census0 = 0, census1 = 0, census2 = 0, census3 = 0, topE = 0, topS = 0, helped = 0, nested = 0, boxes = 0, pairFetches = 0, itersAll = 0, itersGeneral = 0;

    bool haveRay = false;
    int kind = 0;                 // 0: extension ray, 1: shadow ray; 2 / 3: the same, PARKED for the exact walk
    uint32_t index = 0;
    RayPk ray; ray_set(ray, mk3(0, 0, 0), mk3(1, 1, 1));   // origin, direction and 1 / d of the lane's ray
    float distance = kFltMax;     // extension: closest hit so far; shadow: distance of the light
    float hu = 0.0f, hv = 0.0f;
    int hitRef = -1;              // extension: triangle record of the closest hit; shadow: >= 0 when occluded
    bool redo = false;            // the wide walk does not decide this ray: its closest hit ties with a hit of another triangle, or a stack ran full
    int cur = kDone;              // >= 0: WNode to visit; kDone: nothing in hand
    uint32_t pa = 0;              // inner stack: entries sl[bottom .. pa)
    uint32_t pb = S - 1;          // leaf stack: entries sl(pb .. S - 1], pushed downwards
    uint32_t bottom = 0;          // entries below were given to helper lanes
    int ti = -1;                  // next triangle record of the leaf being tested
    int owner = -1;               // >= 0: this lane walks a subtree given to it by lane `owner` (same ray)
    uint32_t outstanding = 0;     // helpers that have not reported yet
    uint32_t donations = 0;       // subtrees this lane has given away for its current ray
    float tT = kFltMax, uT = 0.0f, vT = 0.0f; int refT = -1; bool redoT = false;   // best result reported by this lane's helpers so far
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gtid = blockIdx.x * kDefBlock + threadIdx.x;

    // the helpers' results into the lane's own, once all of them have reported (any order: the smaller t wins, equal t between two lanes
    // counts as a tie; an occluder found by anybody decides a shadow ray whatever else happened)
#define GMUPT_WIDE_MERGE_OWN() \
    do { if (kind == 0) { redo = redo || redoT || (refT >= 0 && tT == distance); if (refT >= 0 && tT < distance) { distance = tT; hu = uT; hv = vT; hitRef = refT; } } \
         else { if (refT >= 0) hitRef = refT; redo = (redo || redoT) && hitRef < 0; } \
         tT = kFltMax; refT = -1; redoT = false; } while (0)
    // the end of a decided ray in its lane
#define GMUPT_WIDE_FINISH() \
    do { if (kind == 0) IO::finish_closest(p, index, ray_o(ray), ray_d(ray), distance, hu, hv, hitRef >= 0 ? (int)ts.pairRef[hitRef] : -1);   /* hitRef is a pair SLOT */ \
         else IO::finish_any(p, index, hitRef >= 0 ? 1u : 0u); \
         haveRay = false; redo = false; } while (0)

    uint32_t loopCount = 0;
    const unsigned long long tStart = STATS ? wall_clock64() : 0ull;   // (collect_stats: wave lifetimes, share of the drain)
    unsigned long long tDrain = 0ull; uint32_t drainIters = 0, drainBusy = 0;
    for (;;) {
        GMUPT_WATCHDOG()
        const bool leavesEmpty = pb == (uint32_t)(S - 1);
        if (STATS && phase == 2) { if (tDrain == 0ull) tDrain = wall_clock64(); drainIters++; drainBusy += (uint32_t)__popcll(__ballot(haveRay)); }
        if (phase == 2) { // wave-uniform: drain service
            // (a) helpers that have finished their subtree (and have heard from their own helpers) report to their owner
            const bool reports = haveRay && owner >= 0 && outstanding == 0u && cur == kDone && leavesEmpty && ti < 0;
            if (reports) GMUPT_WIDE_MERGE_OWN();
            unsigned long long fin = __ballot(reports);
            while (fin) {
                const int hl = __builtin_ctzll(fin); fin &= fin - 1ull;
                GMUPT_HELPER_REPORT()
                const int redoh = __builtin_amdgcn_readlane((int)redo, hl);
                if ((int)lane == ol) {
                    outstanding--;
                    redoT = redoT || redoh != 0;
                    if (rh >= 0) {
                        if (kind == 1) refT = rh;                                                       // any occluder decides a shadow ray
                        else if (th < tT) { tT = th; uT = uh; vT = vh; refT = rh; }
                        else if (th == tT) redoT = true;                                                // a tie parks the ray
                    }
                }
                if ((int)lane == hl) { haveRay = false; owner = -1; tT = kFltMax; refT = -1; redoT = false; redo = false; }
            }
        }
        {   // a lane whose own walk has ended and whose helpers have all reported knows its result -- or that the wide walk did not decide
            // the ray: then the ray is PARKED in the lane (not idle, not free) until the exact walk below takes it
            const bool ended = haveRay && kind < 2 && owner < 0 && outstanding == 0u && cur == kDone && leavesEmpty && ti < 0;
            if (ended) { GMUPT_WIDE_MERGE_OWN(); if (redo) { kind += 2; redo = false; pa = 0; bottom = 0; } }
        }
        if (phase == 2) { // wave-uniform: drain service, continued
            // (b) owners that are done and have heard from all their helpers are written back now: their lanes become free
            const bool done = haveRay && kind < 2 && owner < 0 && outstanding == 0u && cur == kDone && leavesEmpty && ti < 0;
            // (a lane whose walk has ended never gives: an occluded shadow ray leaves its stack behind, and those subtrees no longer matter)
            const unsigned long long wantHelp = __ballot(haveRay && cur != kDone && pa > bottom && donations < 12u);
            if (wantHelp != 0ull && done) GMUPT_WIDE_FINISH();
            // (c) free lanes take the bottom inner entry of lanes that still have some (drain_pair)
            const unsigned long long freeLanes = __ballot(!haveRay);
            if (wantHelp != 0ull && freeLanes != 0ull) {
                const DrainPair pr = drain_pair(wantHelp, freeLanes, lane, haveRay);
                int node = 0;
                if (pr.gives) {
                    node = sl[bottom * kDefBlock];
                    bottom++; outstanding++; donations++;
                    if (STATS) { helped++; if (owner >= 0) nested++; }
                }
                GMUPT_DRAIN_SOURCE(pr, srcLane)
                const int node2 = __shfl(node, srcLane), k2 = __shfl(kind, srcLane), i2 = __shfl((int)index, srcLane);
                const float ox = __shfl(ray.oxy.x, srcLane), oy = __shfl(ray.oxy.y, srcLane), oz = __shfl(ray.ozi.x, srcLane), dx = __shfl(ray.dxy.x, srcLane), dy = __shfl(ray.dxy.y, srcLane), dz = __shfl(ray.dzz.x, srcLane);
                const float lim = __shfl(distance, srcLane);
                if (pr.takes) {
                    haveRay = true; owner = src; kind = k2; index = (uint32_t)i2; donations = 0;
                    ray_set(ray, mk3(ox, oy, oz), mk3(dx, dy, dz));
                    distance = k2 == 1 ? lim : kFltMax;     // shadow: the distance of the light; extension: no hit yet
                    hitRef = -1; hu = 0.0f; hv = 0.0f; redo = false;
                    pa = 0; bottom = 0; pb = S - 1; outstanding = 0; ti = -1;
                    tT = kFltMax; refT = -1; redoT = false;
                    cur = node2;
                }
            }
        }
        // (a helper, a lane that still waits for its helpers, or a parked lane is not idle)
        const bool parked = haveRay && kind >= 2;
        const bool idle = (cur == kDone) && (pb == (uint32_t)(S - 1)) && (ti < 0) && !(haveRay && (owner >= 0 || outstanding != 0u || kind >= 2));
        const unsigned long long idleMask = __ballot(idle);
        const int nIdle = __popcll(idleMask);
        const unsigned long long parkedMask = __ballot(parked);
        if (parkedMask != 0ull) {
            const int nParked = __popcll(parkedMask);
            if (nParked >= kWidePark || nParked + nIdle == 64) {   // wave-uniform
                // ---- the exact walk of the parked rays, as the reference walks them: binary tree, nearer child first, the farther one deferred,
                // triangles of a leaf in order, strict `t < distance` (extensionRayCast.hlsl:96-166); any occluder within the light's distance for a
                // shadow ray (shadowRayCast.hlsl:65-136).  Packed binary copy (Node64 / Tri48); stack = the lane's LDS share, then the global overflow.
                if (lane == 0u) atomicAdd(&p.stats->castRedoRays, (unsigned long long)nParked);
                if (parked) {
                    const bool shadowRay = kind == 3;
                    ray_set(ray, shadowRay ? IO::ray3(p, F_SH_OX, index) : IO::ray3(p, F_RAY_OX, index), shadowRay ? IO::ray3(p, F_SH_DX, index) : IO::ray3(p, F_RAY_DX, index));
                    distance = shadowRay ? IO::rayf(p, F_LIGHT_DIST, index) : IO::closest_limit(p, index);
                    const f3 o = ray_o(ray), invdir = ray_inv(ray), d = ray_d(ray);
                    hitRef = -1; hu = 0.0f; hv = 0.0f;
                    int* ovf = p.ovfStack + gtid;
                    uint32_t sp = 0;
#define GMUPT_EXACT_PUSH(V) do { if (sp < (uint32_t)S) sl[sp * kDefBlock] = (V); else if (sp - (uint32_t)S < (uint32_t)kWideOvf) ovf[(size_t)(sp - (uint32_t)S) * p.ovfStride] = (V); \
                                 else atomicOr(&p.stats->stackOverflow, 1u); sp++; } while (0)
#define GMUPT_EXACT_POP(DST) do { --sp; if (sp < (uint32_t)S) DST = sl[sp * kDefBlock]; else if (sp - (uint32_t)S < (uint32_t)kWideOvf) DST = ovf[(size_t)(sp - (uint32_t)S) * p.ovfStride]; else DST = kDone; } while (0)
                    GMUPT_EXACT_PUSH(kDone);
                    int c = (ray_box(ts.rootMin[0], ts.rootMin[1], ts.rootMin[2], ts.rootMax[0], ts.rootMax[1], ts.rootMax[2], o, invdir) > 0.0f) ? ts.rootDesc : kDone;
                    while (c != kDone) {
                        if (c >= 0) {
                            const Node64& nd = ts.nodes[c];
                            const float leftHit = ray_box(nd.a[0], nd.a[1], nd.a[2], nd.a[3], nd.b[0], nd.b[1], o, invdir);
                            const float rightHit = ray_box(nd.b[2], nd.b[3], nd.c[0], nd.c[1], nd.c[2], nd.c[3], o, invdir);
                            const bool l = leftHit > 0.0f, r = rightHit > 0.0f;
                            const bool swap = leftHit > rightHit;                 // extensionRayCast.hlsl:136
                            const int dl = nd.d[0], dr = nd.d[1];
                            if (l && r) { GMUPT_EXACT_PUSH(swap ? dl : dr); c = swap ? dr : dl; }
                            else if (l | r) c = l ? dl : dr;
                            else GMUPT_EXACT_POP(c);
                        } else {
                            int tix = ~c;
                            bool decided = false;
                            for (;;) {
                                float t = 0.0f, u = 0.0f, v = 0.0f; bool last;
                                if (tri_test(ts.tris, tix, o, d, t, u, v, last)) {
                                    if (shadowRay) { if (t > kEpsilon && t < 1.0f / kEpsilon && length3(d * t) < distance) { hitRef = tix; decided = true; break; } }   // shadowRayCast.hlsl:41-45,89
                                    else if (t >= 0.0f && t < distance) { distance = t; hitRef = tix; hu = u; hv = v; }                                              // extensionRayCast.hlsl:64-74
                                }
                                if (last) break;
                                tix++;
                            }
                            if (decided) c = kDone; else GMUPT_EXACT_POP(c);
                        }
                    }
#undef GMUPT_EXACT_PUSH
#undef GMUPT_EXACT_POP
                    if (shadowRay) IO::finish_any(p, index, hitRef >= 0 ? 1u : 0u);
                    else IO::finish_closest(p, index, o, d, distance, hu, hv, hitRef);
                    haveRay = false; kind = 0; redo = false; cur = kDone; pa = 0; bottom = 0; pb = S - 1; ti = -1;
                    tT = kFltMax; refT = -1; redoT = false; hitRef = -1;
                }
                continue;
            }
        }
        if (nIdle == 64 || (nIdle >= (int)p.tuneRefill && phase < 2)) { // wave-uniform
            GMUPT_CLAIM_CHUNK(IO::entry, p.wideQuarterTail)   // (the last half round in quarter chunks: large tables only)
            GMUPT_CHUNK_SHUFFLE()
            if (idle) {
                // the next ray first: its loads are in flight while the finished ray is written back
                GMUPT_CHUNK_ENTRY()
                const bool newRay = take && (phase != 0 || newIndex != kQueueHole); // holes only exist in the extension queue
                f3 newO = mk3(0, 0, 0), newD = mk3(0, 0, 1); float newDist = kFltMax;
                if (newRay) {
                    if (phase == 0) { newO = IO::ray3(p, F_RAY_OX, newIndex); newD = IO::ray3(p, F_RAY_DX, newIndex); newDist = IO::closest_limit(p, newIndex); }  // :213-214
                    else { newO = IO::ray3(p, F_SH_OX, newIndex); newD = IO::ray3(p, F_SH_DX, newIndex); newDist = IO::rayf(p, F_LIGHT_DIST, newIndex); }         // :162-164
                }
                if (haveRay) GMUPT_WIDE_FINISH();   // (decided: a ray that needs the exact walk was parked at the top of the loop and its lane is not idle)
                if (newRay) {
                    bottom = 0; donations = 0;
                    haveRay = true; kind = phase; index = newIndex;            // phase is 0 (extension) or 1 (shadow) here
                    if (STATS) { if (phase == 0) raysE++; else raysS++; }
                    distance = newDist;
                    ray_set(ray, newO, newD);
                    hitRef = -1; hu = 0.0f; hv = 0.0f; redo = false;
                    pa = 0; pb = S - 1; ti = -1;
                    cur = (ray_box(ts.rootMin[0], ts.rootMin[1], ts.rootMin[2], ts.rootMax[0], ts.rootMax[1], ts.rootMax[2], newO, ray_inv(ray)) > 0.0f) ? 0 : kDone;   // WNode 0 is the root's
                }
            }
            if (nIdle == 64 && phase == 2) break; // nothing in flight and both queues are exhausted (wave-uniform)
            GMUPT_CHUNK_ADVANCE()
        }

        // ---- REPS steps; a burst (wave-uniform, decided once per iteration) adds one triangle test per step to the lanes with leaves pending
        const bool pendingNow = (pb != (uint32_t)(S - 1)) || (ti >= 0);
        const bool roomNow = pb >= pa && pb - pa >= (uint32_t)(kWideRoom - 1);
        if (cur >= 0 && !roomNow && !pendingNow) {
            // the inner stack alone fills the LDS share of this lane: this ray's wide walk is given up, the exact walk (which spills) takes it
            redo = true; cur = kDone; pa = bottom;
        }
        const int nPending = __popcll(__ballot(pendingNow));
        const int nWalking = __popcll(__ballot(cur >= 0 && roomNow));
        const bool burst = nPending >= (int)p.tuneTriThresh || (nWalking == 0 && nPending > 0); // wave-uniform
        if (STATS) { // lane census: where do the 64 lanes of a wave spend the loop iterations?
            census0 += __popcll(__ballot(cur == kDone && !pendingNow)); census1 += __popcll(__ballot(cur >= 0 && roomNow));
            census2 += __popcll(__ballot(cur >= 0 && !roomNow)); census3 += __popcll(__ballot(cur == kDone && pendingNow));
        }
        // (wave-uniform, once per iteration: rays only change in the refill above) the ordered slab tree needs every walking ray's 1 / d finite
        const bool generalSlabs = __ballot(cur >= 0 && (ray_sg(ray) >> 24) != 0u) != 0ull;
        if (STATS && lane == 0u) { itersAll++; if (generalSlabs) itersGeneral++; }
#pragma unroll
        for (int rep = 0; rep < REPS; rep++) {
            // the four slab tests of the node in q0 .. lk, then: the hits are pushed (inner nodes from the bottom, leaves from the top) by
            // "store at the top, advance the top by the predicate" -- eight unconditional LDS stores, no region and no rank per slot -- and
            // the LAST hit inner slot, still in its register, is the next node (why no store destroys a live entry: the head of this file)
#define GMUPT_WIDE_NODE_COMPUTE(INTOP) \
            { if (STATS) { if (kind == 0) tcE.inner++; else tcS.inner++; if (prefix_rank(__ballot(1)) == 0) { if (phase == 0) wInE++; else wInS++; } \
                           if (INTOP) { if (kind == 0) topE++; else topS++; } boxes += (uint32_t)ts.wnodes[cur].aux[1]; } \
              bool h0, h1, h2, h3; \
              slab_hits4(q0, q1, q2, q3, q4, q5, ray, h0, h1, h2, h3, generalSlabs); \
              const bool i0 = h0 & (lk.x >= 0), i1 = h1 & (lk.y >= 0), i2 = h2 & (lk.z >= 0), i3 = h3 & (lk.w >= 0); \
              const bool f0 = h0 & (lk.x < 0), f1 = h1 & (lk.y < 0), f2 = h2 & (lk.z < 0), f3_ = h3 & (lk.w < 0); \
              const uint32_t pa0 = pa, pb0 = pb; \
              sl[pa * kDefBlock] = lk.x; pa += i0 ? 1u : 0u; \
              sl[pa * kDefBlock] = lk.y; pa += i1 ? 1u : 0u; \
              sl[pa * kDefBlock] = lk.z; pa += i2 ? 1u : 0u; \
              sl[pa * kDefBlock] = lk.w; pa += i3 ? 1u : 0u; \
              sl[pb * kDefBlock] = lk.x; pb -= f0 ? 1u : 0u; \
              sl[pb * kDefBlock] = lk.y; pb -= f1 ? 1u : 0u; \
              sl[pb * kDefBlock] = lk.z; pb -= f2 ? 1u : 0u; \
              sl[pb * kDefBlock] = lk.w; pb -= f3_ ? 1u : 0u; \
              if (STATS) { const uint32_t cL = pb0 - pb; if (kind == 0) tcE.leaves += cL; else tcS.leaves += cL; } \
              int nxt = i3 ? lk.w : (i2 ? lk.z : (i1 ? lk.y : lk.x));                                                            /* the last hit inner slot is the next node */ \
              if (pa != pa0) pa--;                                                                                               /* (it is the entry on top: never read back) */ \
              else if (pa > bottom) { pa--; nxt = sl[pa * kDefBlock]; } else { pa = 0; bottom = 0; nxt = kDone; }               /* (an empty inner stack frees its dead entries) */ \
              cur = nxt; }
            vec4f q0, q1, q2, q3, q4, q5; vec4i lk;
            // fetch phase
            const bool doNode = cur >= 0 && pb >= pa && pb - pa >= (uint32_t)(kWideRoom - 1);
            const bool inTop = (uint32_t)cur < topCount;
            const PlaneAddr pla = plane_addresses(cur, ray_sg(ray));    // (for every lane: the node-less ones load nothing)
            if (doNode && inTop) load_wnode_lds_signed(s_top, pla, q0, q1, q2, q3, q4, q5, lk);
            asm volatile("" ::: "memory");   // LDS lanes first, see load_node
            if (doNode && !inTop) load_wnode_glb_signed(rNodes, pla, q0, q1, q2, q3, q4, q5, lk);
            if (burst && ti < 0 && pb != (uint32_t)(S - 1)) { pb++; ti = ~sl[pb * kDefBlock]; }
            const bool doTri = burst && ti >= 0;
            vec4f a0, a1, a2, a3, a4;                        // defined for the doTri lanes only: the TriPair of this step
            if (doTri) {
                const int off = ti * 80;
                a0 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(rPairs, off, 0, 0));
                a1 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(rPairs, off + 16, 0, 0));
                a2 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(rPairs, off + 32, 0, 0));
                a3 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(rPairs, off + 48, 0, 0));
                a4 = __builtin_bit_cast(vec4f, __builtin_amdgcn_raw_buffer_load_b128(rPairs, off + 64, 0, 0));
            }
            // compute phase
            if (doNode) GMUPT_WIDE_NODE_COMPUTE(inTop)
            if (doTri) {
                if (STATS) { pairFetches++; if (prefix_rank(__ballot(1)) == 0) { if (phase == 0) wTrE++; else wTrS++; } }
                const PairHit h = tri_pair_compute(a0, a1, a2, a3, a4, ray);
                bool last = h.last;
                if (STATS) { const uint32_t n = __builtin_bit_cast(vec4u, a4).w; if (kind == 0) tcE.tris += n; else tcS.tris += n; }   // references in this pair (1 or 2; 0 in the pair of an empty leaf)
                if (kind == 0) {
                    // extensionRayCast.hlsl:64-74 for the first, then for the second triangle (a closer hit ends a tie; equal t against another triangle is one)
#define GMUPT_WIDE_ACCEPT(OK, T, U, V, SLOT) \
                    if (OK) { if ((T) >= 0.0f && (T) < distance) { distance = (T); hitRef = (SLOT); hu = (U); hv = (V); redo = false; } \
                              else if ((T) == distance && hitRef >= 0) { if (tri_canon(rTris, (int)ts.pairRef[SLOT]) != tri_canon(rTris, (int)ts.pairRef[hitRef])) redo = true; } }
                    GMUPT_WIDE_ACCEPT(h.okA, h.t.x, h.u.x, h.v.x, 2 * ti)
                    GMUPT_WIDE_ACCEPT(h.okB, h.t.y, h.u.y, h.v.y, 2 * ti + 1)
#undef GMUPT_WIDE_ACCEPT
                } else {
                    // shadowRayCast.hlsl:41-45,89: t in (1e-8, 1e8) and |d t| < lightDistance => occluded: the ray is decided
                    const f3 d = ray_d(ray);
                    const bool occA = h.okA && h.t.x > kEpsilon && h.t.x < 1.0f / kEpsilon && length3(d * h.t.x) < distance;
                    const bool occB = h.okB && h.t.y > kEpsilon && h.t.y < 1.0f / kEpsilon && length3(d * h.t.y) < distance;
                    if (occA | occB) { hitRef = 2 * ti; last = true; pb = S - 1; cur = kDone; pa = bottom; redo = false; }
                }
                ti = last ? -1 : ti + 1;
            }
        }
    }
#undef GMUPT_WIDE_MERGE_OWN
#undef GMUPT_WIDE_FINISH
#undef GMUPT_WIDE_NODE_COMPUTE
    if (STATS) { flush_cast_counts(p.stats, tcE, raysE, wInE, wTrE, tcS, raysS, wInS, wTrS, topE, topS, helped, nested);
                 flush_sum(&p.stats->wideBoxTests, boxes); flush_sum(&p.stats->wideIters, itersAll); flush_sum(&p.stats->wideGeneralIters, itersGeneral); flush_sum(&p.stats->widePairFetches, pairFetches);
                 if (lane == 0u) {
                     atomicAdd(&p.stats->castWaves, 1ull); const unsigned long long tEnd = wall_clock64();
                     flush_drain_share(p.stats, tEnd, tDrain, drainIters, drainBusy);
                     flush_wave_life(p.stats, tEnd - tStart, census0, census1, census2, census3);
                 } }
}

// ------------------------------------------------------------------------------------------------ host launchers
uint32_t traversal_wide_top_capacity() { return (uint32_t)kWideTop; }
uint32_t traversal_wide_stack_entries() { return (uint32_t)kWideStack; }
uint32_t traversal_wide_overflow_entries() { return (uint32_t)kWideOvf; }

// Steps per iteration of a wave (between two looks at the queues): six while the records fit the 256 MB Infinity Cache, eight beyond
// (measured: config 3 0.923 / 0.930 ms with six / eight, config 5 5.12 / 5.00 ms); GMUPT_WIDE_STEPS overrides.  With eight steps the last
// half round of shadow-ray chunks is handed out in quarters (measured with it: config 5 4.87-4.95 vs 4.95-4.99 ms, config 3 0.926-0.928
// vs 0.920-0.923).  Sets q.wideQuarterTail; returns whether the eight-step kernel is the one to launch.
static bool wide_eight_steps(RenderParams& q)
{
    const uint64_t recordBytes = (uint64_t)q.trav.wideCount * 128ull + (uint64_t)q.trav.numPairs * 80ull;
    const bool eight = q.tuneWideSteps ? q.tuneWideSteps >= 8u : recordBytes > (256ull << 20);
    q.wideQuarterTail = eight ? 1u : 0u;
    return eight;
}

// Both ray casts in one wide launch.  Returns 0 when this configuration is not taken (the caller runs another kernel).
uint32_t launch_cast_wide(const RenderParams& p, bool stats, hipStream_t s)
{
    if (!p.trav.wnodes || p.extendPrune || p.shadowPrune) return 0u;
    if (!wide_tables_addressable(p.trav.wideCount, p.scene.numTris, p.trav.numPairs)) return 0u;
    const uint32_t pb = p.travGridBlocks;
    RenderParams q = p;
    const bool eight = wide_eight_steps(q);
    if (stats) { if (eight) hipLaunchKernelGGL((k_cast_w<true, GMUPT_WIDE_REPS + 2, StateIO>), dim3(pb), dim3(kDefBlock), 0, s, q); else hipLaunchKernelGGL((k_cast_w<true, GMUPT_WIDE_REPS, StateIO>), dim3(pb), dim3(kDefBlock), 0, s, q); }
    else { if (eight) hipLaunchKernelGGL((k_cast_w<false, GMUPT_WIDE_REPS + 2, StateIO>), dim3(pb), dim3(kDefBlock), 0, s, q); else hipLaunchKernelGGL((k_cast_w<false, GMUPT_WIDE_REPS, StateIO>), dim3(pb), dim3(kDefBlock), 0, s, q); }
    return GMUPT_STAT_FUSED_CAST | GMUPT_STAT_CAST_WIDE;
}

// gmupt_trace_rays: the same walk over caller rays (QueryIO).  p is the renderer's parameter block with p.stats and p.travCounters
// already pointing at the query's own zeroed buffers (gmupt_capi.hip checks that the scene has a wide collapse within the 2 GiB limits).
// The rest of the launch is launch_cast_wide's: grid, overflow stacks, steps per iteration and tail rule (wide_eight_steps).
void launch_trace_wide(const RenderParams& p, const gmupt_ray* closest, uint32_t nClosest, gmupt_hit* hits, const gmupt_ray* any, uint32_t nAny,
                       uint32_t* occluded, uint32_t lightCount, hipStream_t s)
{
    QueryParams q;
    static_cast<RenderParams&>(q) = p;
    q.rays[0] = closest; q.rays[1] = any; q.count[0] = nClosest; q.count[1] = nAny;
    q.hits = hits; q.occluded = occluded; q.lightCount = lightCount;
    if (wide_eight_steps(q)) hipLaunchKernelGGL((k_cast_w<false, GMUPT_WIDE_REPS + 2, QueryIO>), dim3(p.travGridBlocks), dim3(kDefBlock), 0, s, q);
    else hipLaunchKernelGGL((k_cast_w<false, GMUPT_WIDE_REPS, QueryIO>), dim3(p.travGridBlocks), dim3(kDefBlock), 0, s, q);
}

} // namespace gmupt
