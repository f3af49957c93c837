// patches.hip -- connected-component patch extraction (S7), per-patch depth maps (S8) and the raw-point
// update (S9) on gfx950.
//
// Replaces PCCPatchSegmenter3::segmentPatches (reference: source/lib/PccLibEncoder/source/
// PCCPatchSegmenter.cpp:542-1320, CTC branch: no EOM / patch expansion / partitioning / gradient
// separation) together with resampledPointcloud (:362-470) and the per-round k-d tree + 1-NN (:1291-1298).
//
// S7  The reference floods components sequentially (LIFO over the DIRECTED 16-NN lists, same plane,
//     seeds in increasing index among raw points farther than 9 from the resampled cloud).  The set a
//     seed absorbs is exactly { v : s is the SMALLEST eligible seed that reaches v }, so
//     the components are the fixpoint of label[v] = min(label[v], label[u]) over edges u->v; patch
//     order = increasing label.  Push-style atomicMin sweeps; several sweeps per host round-trip.
// S8  All per-patch quantities are min/max/count reductions (inputs have no duplicate positions), so
//     they are atomics: bbox, then a 64-bit atomicMin/Max of (depth << 32 | point id) per pixel gives D0
//     and its source point in one pass.  Depth maps are processed as 16x16 tiles = one 256-lane
//     workgroup per occupancy block: block peak by wave reduction, outlier filter, D1 seeding, block
//     occupancy by ballot, conversion to patch-local depth.
// S9  Only thresholds of the distance to the resampled cloud matter (> 9 seeds, > 1 stays raw), so the
//     per-round k-d tree is replaced by a dense 3-D occupancy bitmap of the resampled voxels in HBM
//     (2^30 bits = 128 MiB at vox10) probed in increasing-distance order.
#include <algorithm>
#include <cmath>

#include "internal.h"
#include "loads.h"
#include "wave.h"
#include "union_find.h"

namespace tmc2 {
namespace {

using Uf = UnionFind<false>;  // the word of a point is its parent

constexpr uint32_t kNoLabel = 0xFFFFFFFFu;
constexpr uint32_t kFar     = 0xFFFFFFFFu;  // "distance to the resampled cloud unknown / beyond the probe radius"

struct PatchDev {
  int32_t u1, v1, d1;
  int32_t sizeU, sizeV, sizeU0, sizeV0;
  int32_t axN, axT, axB, mode;
  int32_t blockBase;  // first tile of this patch in the round's tile list
  int64_t depthOff;   // into the frame's depth pools
  int64_t occOff;     // into the frame's occupancy pool
};

// Wave-aggregated reductions keyed by a small integer (patch / component id).  Neighbouring points almost always
// share the key, so instead of 64 atomics on one address per wavefront the lanes holding the same key are reduced
// with cross-lane shuffles and ONE lane issues the atomics.  Loops once per distinct key present in the wave.
// All 64 lanes must call these (key < 0 = nothing to contribute).
// A body-sized patch still receives one report per wave (thousands per address): look before the atomic -- the running
// value is monotone, so a stale read can only cause a redundant atomic, never a missed one.
__device__ __forceinline__ void lazyAtomicMin( int32_t* a, int v ) {
  if ( v < loadStaleOk( a ) ) atomicMin( a, v );
}
__device__ __forceinline__ void lazyAtomicMax( int32_t* a, int v ) {
  if ( v > loadStaleOk( a ) ) atomicMax( a, v );
}

// (a point's step fetches its k-NN row, its own words, then its 16 neighbours' words in load batches: loads.h)

// ---- S7 ---------------------------------------------------------------------------------------------
// Connected components of the reference = "smallest eligible seed that reaches v" over the DIRECTED k-NN graph
// restricted to raw points of one plane.  Pushing labels along edges needs as many dependent steps as
// the graph is deep (hundreds of hops on a body-sized patch).  Instead:
//   1. mutual edges (u in knn[v] and v in knn[u]) are bidirectional, so everything they connect is reached by
//      exactly the same seeds: a lock-free union-find over the mutual edges (union_find.h) collapses each such group
//      in O(log) dependent steps;
//   2. lab[root] = smallest ELIGIBLE member (atomicMin);
//   3. the remaining one-way edges connect groups; lab[] is relaxed along them until nothing changes -- on the
//      condensed graph that is a handful of sweeps, each touching only the one-way edges.
// The result is the unique fixpoint, so it does not depend on scheduling.

// bit j of mutual[u] = knn[u][j] lists u in its own row.  Depends only on the adjacency: once per call.
// Every row is read by the point itself and by its (up to) sixteen in-neighbours: 64 N bytes if each row reached HBM once, sixteen
// times that if none stayed cached.  With the blocks as they come every L2 saw every region of the cloud (counters: 325 MB for 55 MB
// of contract bytes); chunked (internal.h: the XCD work mapping) 85 MB.  perm != nullptr: the points in TREE order instead of
// input order (no faster on clouds that arrive in scan order: option MUTUAL_ORDER=tree).
template <int K>
__global__ __launch_bounds__( 256 ) void ccMutualMaskKernel( const uint32_t* __restrict__ knn, const uint32_t* __restrict__ perm, bool chunked,
                                                              uint32_t n, uint16_t* __restrict__ mutual ) {
  const uint32_t at = logicalBlock( chunked ) * blockDim.x + threadIdx.x;
  if ( at >= n ) return;
  const uint32_t u = perm ? perm[at] : at;
  uint32_t     nb[K];
  const uint4* row = reinterpret_cast<const uint4*>( knn + size_t( u ) * K );
#pragma unroll
  for ( int j = 0; j < K / 4; ++j ) {
    const uint4 r = row[j];
    nb[4 * j] = r.x, nb[4 * j + 1] = r.y, nb[4 * j + 2] = r.z, nb[4 * j + 3] = r.w;
  }
  uint32_t m = 0;
#pragma unroll
  for ( int j = 0; j < K; ++j ) {
    const uint32_t v = nb[j];
    if ( v == u ) continue;
    const uint4* rv  = reinterpret_cast<const uint4*>( knn + size_t( v ) * K );
    bool         hit = false;
#pragma unroll
    for ( int t = 0; t < K / 4; ++t ) {
      const uint4 r = rv[t];
      hit |= ( r.x == u ) | ( r.y == u ) | ( r.z == u ) | ( r.w == u );
    }
    m |= hit ? ( 1u << j ) : 0u;
  }
  mutual[u] = uint16_t( m );
}

// The point of this lane in a one-point-per-lane pass of the patch rounds (n: none).  Round 1 (LIST = false): every point is raw and
// the pass runs over all n of them (count == n), in the order its caller chose.  Later rounds: over list[0 .. count), the points
// still raw in ASCENDING index order (rawListScatterKernel), on a grid of count lanes -- a lane per point of the cloud would find
// raw[i] == 0 and leave in nearly all of them.  The arrays indexed by point or seed keep their size and meaning; a pass run from
// the list leaves the entries of the other points as they are, and nothing reads them (segmentPatches: which consumers).
template <bool LIST>
__device__ __forceinline__ uint32_t roundPoint( const uint32_t* __restrict__ list, uint32_t count, uint32_t n ) {
  const uint32_t j = chunkedIndex();
  if ( LIST ) return j < count ? list[j] : n;
  return j < n ? j : n;
}
template <bool LIST>
__device__ __forceinline__ uint32_t roundPoint( const uint32_t* __restrict__ list, uint32_t count, const uint32_t* __restrict__ perm,
                                                bool chunked, uint32_t n ) {
  return LIST ? roundPoint<true>( list, count, n ) : pointOfLane( perm, chunked, n );
}

// Initial forest without atomics: every raw point hooks itself under the eligible mutual neighbour of smallest hashed
// priority, if smaller than its own (priorities strictly decrease along parent links: acyclic).  Most unions are done
// before the first compare-and-swap, and the paths the union pass walks end at local priority minima.
template <bool LIST, int K>
__global__ __launch_bounds__( 256 ) void ccInitKernel( const uint32_t* __restrict__ knn, const uint16_t* __restrict__ mutual,
                                                        const uint8_t* __restrict__ partition, const uint8_t* __restrict__ raw,
                                                        const uint32_t* __restrict__ perm, bool chunked,
                                                        const uint32_t* __restrict__ list, uint32_t count, uint32_t n,
                                                        uint32_t* __restrict__ parent, uint32_t* __restrict__ lab,
                                                        uint32_t* __restrict__ ccCount ) {
  const uint32_t i = roundPoint<LIST>( list, count, perm, chunked, n );
  if ( i >= n ) return;
  static_assert( K == 16, "the row is read as four 16-byte loads" );
  lab[i]     = kNoLabel;
  ccCount[i] = 0;
  // trip 1: everything indexed by the point alone, the whole row included
  Words4 r[4];
  loadRow16( knn, i, r );
  uint32_t rawI = raw[i], m = mutual[i], pi = partition[i];
  pin( r[0], r[1], r[2], r[3], rawI, m, pi );
  uint32_t v[K];
  rowEntries( r, v );
  if ( !rawI ) m = 0;
  // trip 2: raw and plane of the masked (mutual) neighbours -- row entries: valid indices whatever the point's own state
  uint32_t rawV[K], partV[K];
#pragma unroll
  for ( int j = 0; j < K; ++j ) {
    rawV[j] = 0, partV[j] = 0;
    if ( ( m >> j ) & 1u ) rawV[j] = raw[v[j]], partV[j] = partition[v[j]];
  }
  pinAll( rawV );
  pinAll( partV );
  // the choice: ascending j, strict <, as the serial loop over the set bits made it
  uint32_t best = i, bestPrio = ufPriority( i );
#pragma unroll
  for ( int j = 0; j < K; ++j )
    if ( ( ( m >> j ) & 1u ) && ufPriority( v[j] ) < bestPrio && rawV[j] && partV[j] == pi ) {
      best     = v[j];
      bestPrio = ufPriority( v[j] );
    }
  parent[i] = best;
}

// The unions over the eligible mutual edges (raw ends of one plane); the union-find itself: union_find.h.
template <bool LIST, int K>
__global__ __launch_bounds__( 256 ) void ccUnionKernel( const uint32_t* __restrict__ knn, const uint16_t* __restrict__ mutual,
                                                         const uint8_t* __restrict__ partition,
                                                         const uint8_t* __restrict__ raw, const uint32_t* __restrict__ perm,
                                                         bool chunked, const uint32_t* __restrict__ list, uint32_t count, uint32_t n,
                                                         uint32_t* __restrict__ parent, int precheck, bool agent ) {
  const uint32_t u = roundPoint<LIST>( list, count, perm, chunked, n );
  if ( u >= n || !raw[u] ) return;
  uint32_t m = mutual[u];
  if ( !m ) return;
  const uint8_t   pu  = partition[u];
  const uint32_t* row = knn + size_t( u ) * K;
  while ( m ) {
    const int j = __ffs( int( m ) ) - 1;
    m &= m - 1;
    const uint32_t v = row[j];
    if ( v > u || !raw[v] || partition[v] != pu ) continue;  // every mutual edge is seen from both ends: larger one acts
    if ( precheck && Uf::sameSetStale( parent, u, v, agent ) ) continue;
    Uf::unite( parent, u, v, 0u, agent );
  }
}

// Debug invariants of the settled forest (TMC2_UF_CHECK=1, the soak tests): every link goes to a raw point of the same plane
// and of smaller priority; the two ends of every eligible mutual edge have one root (Uf::rootCoherent).  bad[0] = broken
// links, bad[1] = edges whose ends ended up in different sets.
template <bool LIST, int K>
__global__ __launch_bounds__( 256 ) void ccCheckKernel( const uint32_t* __restrict__ knn, const uint16_t* __restrict__ mutual,
                                                         const uint8_t* __restrict__ partition, const uint8_t* __restrict__ raw,
                                                         const uint32_t* __restrict__ list, uint32_t count, uint32_t n, uint32_t* parent,
                                                         uint32_t* __restrict__ bad ) {
  const uint32_t at = blockIdx.x * blockDim.x + threadIdx.x;
  if ( at >= count ) return;
  const uint32_t u = LIST ? list[at] : at;
  if ( u >= n || !raw[u] ) return;
  const uint32_t p = __hip_atomic_load( &parent[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
  if ( p != u && ( p >= n || !raw[p] || partition[p] != partition[u] || ufPriority( p ) >= ufPriority( u ) ) ) atomicAdd( &bad[0], 1u );
  const uint32_t ru = Uf::rootCoherent( parent, u, n );
  if ( ru == kUfBroken ) {
    atomicAdd( &bad[0], 1u );
    return;
  }
  uint32_t m = mutual[u];
  while ( m ) {
    const int j = __ffs( int( m ) ) - 1;
    m &= m - 1;
    const uint32_t v = knn[size_t( u ) * K + j];
    if ( v > u || !raw[v] || partition[v] != partition[u] ) continue;
    if ( Uf::rootCoherent( parent, v, n ) != ru ) atomicAdd( &bad[1], 1u );
  }
}

template <bool LIST>
__global__ __launch_bounds__( 256 ) void ccFlattenSeedKernel( const uint8_t* __restrict__ raw, const uint32_t* __restrict__ dist,
                                                               uint32_t thrDetection, const uint32_t* __restrict__ list,
                                                               uint32_t count, uint32_t n, uint32_t* __restrict__ parent,
                                                               uint32_t* __restrict__ root, uint32_t* __restrict__ lab, bool agent ) {
  const uint32_t u    = roundPoint<LIST>( list, count, n );
  const int      lane = threadIdx.x & 63;
  uint32_t       r    = kNoLabel;
  bool           seed = false;
  if ( u < n && raw[u] ) {
    r       = Uf::find( parent, u, agent ).root;  // (the flat view goes to its own array: union_find.h)
    root[u] = r;
    seed    = dist[u] > thrDetection;
  }
  // a body-sized group has hundreds of thousands of members: one atomic per wave and group, and only if it can lower
  unsigned long long todo = __ballot( seed );
  while ( todo ) {
    const int                leader = __ffsll( (long long)todo ) - 1;
    const uint32_t           key    = __shfl( r, leader, 64 );
    const unsigned long long same   = __ballot( seed && r == key );
    // lanes are in index order (the list is ascending), so the leader (lowest lane of its group) holds the group's smallest index
    // in the wave
    if ( lane == leader && loadStaleOk( &lab[key], agent ) > u )
      atomicMin( &lab[key], u );
    todo &= ~same;
  }
}

// one relaxation sweep over the one-way edges between groups (parent = the flat roots ccFlattenSeedKernel wrote)
template <bool LIST, int K>
__global__ __launch_bounds__( 256 ) void ccRelaxKernel( const uint32_t* __restrict__ knn, const uint16_t* __restrict__ mutual,
                                                         const uint8_t* __restrict__ partition,
                                                         const uint8_t* __restrict__ raw, const uint32_t* __restrict__ parent,
                                                         const uint32_t* __restrict__ perm, bool chunked,
                                                         const uint32_t* __restrict__ list, uint32_t count, uint32_t n,
                                                         uint32_t* __restrict__ lab, uint32_t* __restrict__ changed, uint32_t token,
                                                         bool agent ) {
  const uint32_t u = roundPoint<LIST>( list, count, perm, chunked, n );
  static_assert( K == 16, "the row is read as four 16-byte loads" );
  if ( u >= n ) return;
  // trip 1: everything indexed by the point alone (parent[u] of a point that is not raw is stale: it goes nowhere, below)
  Words4 r[4];
  loadRow16( knn, u, r );
  uint32_t rawU = raw[u], mu = mutual[u], ru = parent[u], pu = partition[u];
  pin( r[0], r[1], r[2], r[3], rawU, mu, ru, pu );
  uint32_t m = ~mu & ( ( 1u << K ) - 1u );
  if ( !rawU || !m ) return;
  uint32_t v[K];
  rowEntries( r, v );
  // trip 2: the point's label, and raw and plane of every one-way neighbour (row entries: valid indices)
  uint32_t lu = loadStaleOk( &lab[ru], agent );
  uint32_t rawV[K], partV[K];
#pragma unroll
  for ( int j = 0; j < K; ++j ) {
    rawV[j] = 0, partV[j] = 0;
    if ( ( m >> j ) & 1u ) rawV[j] = raw[v[j]], partV[j] = partition[v[j]];
  }
  pin( lu );
  pinAll( rawV );
  pinAll( partV );
  if ( lu == kNoLabel ) return;
  uint32_t elig = 0;
#pragma unroll
  for ( int j = 0; j < K; ++j )
    elig |= uint32_t( ( v[j] != u ) & ( rawV[j] != 0 ) & ( partV[j] == pu ) ) << j;  // (the predicates of the serial loop)
  elig &= m;
  if ( !elig ) return;
  // trip 3: the flat root of the eligible neighbours (raw points of this round: written by ccFlattenSeedKernel)
  uint32_t rv[K];
#pragma unroll
  for ( int j = 0; j < K; ++j ) {
    rv[j] = ru;
    if ( ( elig >> j ) & 1u ) rv[j] = parent[v[j]];
  }
  pinAll( rv );
  // trip 4: their labels
  uint32_t lv[K];
#pragma unroll
  for ( int j = 0; j < K; ++j ) {
    lv[j] = 0;
    if ( rv[j] != ru ) lv[j] = loadStaleOk( &lab[rv[j]], agent );
  }
  pinAll( lv );
  // the pushes: every one issued before an answer is looked at (atomicMin and the token do not depend on the order)
#pragma unroll
  for ( int j = 0; j < K; ++j ) {
    const uint32_t seen = lv[j];
    lv[j]               = 0;
    if ( rv[j] != ru && seen > lu ) lv[j] = atomicMin( &lab[rv[j]], lu );
  }
  pinAll( lv );
  bool any = false;
#pragma unroll
  for ( int j = 0; j < K; ++j ) any |= lv[j] > lu;
  if ( any ) *changed = token;  // (which sweep changed something last: nothing to clear between sweeps)
}

// start of a round's per-patch accumulators: bounding box {min 3 x INT_MAX, max 3 x 0 -- the reference starts its max at 0},
// minimum (u, v), the two resampling counters
__global__ __launch_bounds__( 256 ) void patchBoundsInitKernel( uint32_t P, int32_t* __restrict__ bbox, int32_t* __restrict__ minUv,
                                                                 int32_t* __restrict__ patchStat ) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if ( p >= P ) return;
#pragma unroll
  for ( int d = 0; d < 3; ++d ) {
    bbox[6 * p + d]     = 0x7FFFFFFF;
    bbox[6 * p + 3 + d] = 0;
  }
  minUv[2 * p] = minUv[2 * p + 1] = 0x7F7F7F7F;
  patchStat[2 * p] = patchStat[2 * p + 1] = 0;
}

// label of every point still raw (the label of its group), and the size of every component (one atomic per run of equal
// labels in a wavefront)
// (round 6: the sizes are only ever compared with minCount -- ccSeedFlagKernel, ccAssignKernel -- so a component that has reached it
//  stops counting: the body of a figure is ONE component of 10^5 points, and 13 000 wavefronts adding to its one word queued up for
//  ~ 11 ns each; the look is a possibly stale view of a counter that only grows -- a stale read costs an add, never a wrong answer)
template <bool LIST>
__global__ __launch_bounds__( 256 ) void ccLabelCountKernel( const uint8_t* __restrict__ raw, const uint32_t* __restrict__ parent,
                                                              const uint32_t* __restrict__ lab, const uint32_t* __restrict__ list,
                                                              uint32_t count, uint32_t n, uint32_t minCount,
                                                              uint32_t* __restrict__ label, uint32_t* __restrict__ ccCount ) {
  const uint32_t i    = roundPoint<LIST>( list, count, n );
  const int      lane = threadIdx.x & 63;
  const uint32_t l    = ( i < n && raw[i] ) ? lab[parent[i]] : kNoLabel;
  if ( i < n ) label[i] = l;
  unsigned long long todo = __ballot( l != kNoLabel );
  while ( todo ) {
    const int                leader = __ffsll( (long long)todo ) - 1;
    const uint32_t           key    = __shfl( l, leader, 64 );
    const unsigned long long same   = __ballot( l == key );
    if ( lane == leader && loadStaleOk( &ccCount[key] ) < minCount ) atomicAdd( &ccCount[key], uint32_t( __popcll( same ) ) );
    todo &= ~same;
  }
}

// (ccCount is an accumulation: before a round labels again -- later rounds: the counts of the listed points, the only ones a label
//  can name; round 1 clears all n with a memset)
__global__ __launch_bounds__( 256 ) void ccClearCountKernel( const uint32_t* __restrict__ list, uint32_t count,
                                                              uint32_t* __restrict__ ccCount ) {
  const uint32_t j = chunkedIndex();
  if ( j < count ) ccCount[list[j]] = 0;
}

// flag[j] = the j-th point of the pass (round 1: point j) is the seed of a component that becomes a patch; the scan over these gives
// the patches their numbers: rank in ascending seed index, from the list as from all n points
template <bool LIST>
__global__ __launch_bounds__( 256 ) void ccSeedFlagKernel( const uint32_t* __restrict__ label,
                                                            const uint32_t* __restrict__ ccCount, uint32_t minCount,
                                                            const uint32_t* __restrict__ list, uint32_t count,
                                                            uint32_t* __restrict__ flag ) {
  const uint32_t j = chunkedIndex();
  if ( j >= count ) return;
  const uint32_t i = LIST ? list[j] : j;
  flag[j]          = ( label[i] == i && ccCount[i] >= minCount ) ? 1u : 0u;
}

// per point: patch (this round's rank of its component) or -1; per patch: plane of the seed.  posOf[l]: where the list holds point l
// (a label is a seed, a point still raw), which is where the scan left its rank
template <bool LIST>
__global__ __launch_bounds__( 256 ) void ccAssignKernel( const uint32_t* __restrict__ label,
                                                          const uint32_t* __restrict__ ccCount,
                                                          const uint32_t* __restrict__ rank, const uint32_t* __restrict__ posOf,
                                                          const uint8_t* __restrict__ partition, uint32_t minCount,
                                                          const uint32_t* __restrict__ list, uint32_t count, uint32_t n,
                                                          int32_t* __restrict__ pointPatch, int32_t* __restrict__ patchView ) {
  const uint32_t i = roundPoint<LIST>( list, count, n );
  if ( i >= n ) return;
  const uint32_t l = label[i];
  int32_t        p = -1;
  if ( l != kNoLabel && ccCount[l] >= minCount ) {
    p = int32_t( rank[LIST ? posOf[l] : l] );
    if ( l == i ) patchView[p] = partition[i];
  }
  pointPatch[i] = p;
}

// ---- S8 reductions ------------------------------------------------------------------------------------
// stats[p] = { minU, minV } (splitting window anchor)
// Per-patch minima / maxima over the points of a workgroup, in LDS first: a small open-addressing table keyed by patch (LDS
// atomics cost next to nothing and meet no other workgroup), then one look-before-you-atomic per table entry and field.
// Points come in input order -- a wave's 64 points belong to up to dozens of patches -- so reducing patch by patch inside the
// wave (a masked butterfly per field and distinct patch) was 0.13 - 0.3 ms per launch; per-point global atomics would meet on
// the handful of words of a big patch.  A point whose patch finds no slot (more than kAggSlots distinct patches in one
// workgroup) reports to global memory itself.
constexpr int kAggSlots = 128;
template <int FIELDS>
struct PatchAgg {
  int32_t key[kAggSlots];
  int32_t val[kAggSlots][FIELDS];
};
// MINS: the first MINS fields are minima, the others maxima
template <int FIELDS, int MINS>
__device__ __forceinline__ void aggInit( PatchAgg<FIELDS>& t ) {
  for ( int i = threadIdx.x; i < kAggSlots; i += blockDim.x ) {
    t.key[i] = -1;
#pragma unroll
    for ( int k = 0; k < FIELDS; ++k ) t.val[i][k] = k < MINS ? 0x7FFFFFFF : int32_t( 0x80000000 );
  }
  __syncthreads();
}
template <int FIELDS, int MINS>
__device__ __forceinline__ void aggAdd( PatchAgg<FIELDS>& t, int32_t patch, const int ( &v )[FIELDS], int32_t* __restrict__ out ) {
  int slot = int( ( uint32_t( patch ) * 2654435761u ) >> 25 );  // (kAggSlots = 2^7)
  for ( int tries = 0; tries < kAggSlots; ++tries, slot = ( slot + 1 ) & ( kAggSlots - 1 ) ) {
    const int32_t k = atomicCAS( &t.key[slot], -1, patch );
    if ( k == -1 || k == patch ) {
#pragma unroll
      for ( int f = 0; f < FIELDS; ++f ) {
        if ( f < MINS )
          atomicMin( &t.val[slot][f], v[f] );
        else
          atomicMax( &t.val[slot][f], v[f] );
      }
      return;
    }
  }
#pragma unroll
  for ( int f = 0; f < FIELDS; ++f ) {  // no slot left
    if ( f < MINS )
      lazyAtomicMin( &out[FIELDS * patch + f], v[f] );
    else
      lazyAtomicMax( &out[FIELDS * patch + f], v[f] );
  }
}
template <int FIELDS, int MINS>
__device__ __forceinline__ void aggFlush( PatchAgg<FIELDS>& t, int32_t* __restrict__ out ) {
  __syncthreads();
  for ( int i = threadIdx.x; i < kAggSlots * FIELDS; i += blockDim.x ) {
    const int     slot = i / FIELDS, f = i % FIELDS;
    const int32_t k    = t.key[slot];
    if ( k < 0 ) continue;
    if ( f < MINS )
      lazyAtomicMin( &out[FIELDS * k + f], t.val[slot][f] );
    else
      lazyAtomicMax( &out[FIELDS * k + f], t.val[slot][f] );
  }
}

template <bool LIST>
__global__ __launch_bounds__( 256 ) void patchMinUvKernel( const Pt* __restrict__ pts, const int32_t* __restrict__ pointPatch,
                                                            const int32_t* __restrict__ patchView, const uint32_t* __restrict__ list,
                                                            uint32_t count, uint32_t n, int32_t* __restrict__ minUv ) {
  __shared__ PatchAgg<2> agg;
  aggInit<2, 2>( agg );
  const uint32_t i = roundPoint<LIST>( list, count, n );
  const int32_t  p = i < n ? pointPatch[i] : -1;
  if ( p >= 0 ) {
    const int view = patchView[p] % 3;
    const int axT = view == 0 ? 2 : ( view == 1 ? 2 : 0 ), axB = view == 0 ? 1 : ( view == 1 ? 0 : 1 );
    const Pt  q    = pts[i];
    const int uv[2] = {coordOf( q, axT ), coordOf( q, axB )};
    aggAdd<2, 2>( agg, p, uv, minUv );
  }
  aggFlush<2, 2>( agg, minUv );
}

template <bool LIST>
__global__ __launch_bounds__( 256 ) void patchTrimBboxKernel( const Pt* __restrict__ pts, const int32_t* __restrict__ patchView,
                                                               const int32_t* __restrict__ minUv, int splitting,
                                                               int maxPatchSize, const uint32_t* __restrict__ list, uint32_t count,
                                                               uint32_t n, int32_t* __restrict__ pointPatch,
                                                               int32_t* __restrict__ bbox ) {
  __shared__ PatchAgg<6> agg;
  aggInit<6, 3>( agg );
  const uint32_t i = roundPoint<LIST>( list, count, n );
  int32_t        p = -1;
  Words2         qw = {0u, 0u};
  if ( i < n ) p = pointPatch[i], qw = loadPt( pts, i );  // trip 1
  pin( p, qw );
  if ( p >= 0 ) {
    const Pt q = ptOf( qw );
    if ( splitting ) {
      // trip 2: the patch's view with both words of its window anchor (one 8-byte load: 2 p is even, the array starts a pool block)
      int32_t vw = patchView[p];
      Words2  mn = reinterpret_cast<const Words2*>( minUv )[p];
      pin( vw, mn );
      const int view = vw % 3;
      const int axT = view == 0 ? 2 : ( view == 1 ? 2 : 0 ), axB = view == 0 ? 1 : ( view == 1 ? 0 : 1 );
      if ( !( coordOf( q, axT ) - int32_t( mn.x ) < maxPatchSize && coordOf( q, axB ) - int32_t( mn.y ) < maxPatchSize ) ) {
        pointPatch[i] = -1;  // trimmed: stays raw for a later round
        p             = -1;
      }
    }
    if ( p >= 0 ) {
      const int box[6] = {q.x, q.y, q.z, q.x, q.y, q.z};
      aggAdd<6, 3>( agg, p, box, bbox );
    }
  }
  aggFlush<6, 3>( agg, bbox );
}

// D0 candidates: 64-bit (depth << 32 | point) min (mode 0) / max (mode 1) per pixel
template <bool LIST>
__global__ __launch_bounds__( 256 ) void patchDepth0Kernel( const Pt* __restrict__ pts, const int32_t* __restrict__ pointPatch,
                                                             const PatchDev* __restrict__ patches, const uint32_t* __restrict__ list,
                                                             uint32_t count, uint32_t n, int64_t roundDepthBase,
                                                             unsigned long long* __restrict__ map64 ) {
  const uint32_t i = roundPoint<LIST>( list, count, n );
  if ( i >= n ) return;
  const int32_t p = pointPatch[i];
  if ( p < 0 ) return;
  const PatchDev pd = patches[p];
  const Pt       q  = pts[i];
  const int      d = coordOf( q, pd.axN ), u = coordOf( q, pd.axT ) - pd.u1, v = coordOf( q, pd.axB ) - pd.v1;
  const size_t   px  = size_t( pd.depthOff - roundDepthBase ) + size_t( v ) * pd.sizeU + u;
  const unsigned long long val = ( (unsigned long long)uint32_t( d + 1 ) << 32 ) | i;  // +1: 0 stays a sentinel
  if ( pd.mode == 0 )
    atomicMin( &map64[px], val );
  else
    atomicMax( &map64[px], val );
}

// per tile: reset the 64-bit D0 candidates to the projection mode's sentinel
__global__ __launch_bounds__( 256 ) void patchInitTileKernel( const PatchDev* __restrict__ patches,
                                                               const uint32_t* __restrict__ tilePatch,
                                                               int64_t roundDepthBase, int occRes,
                                                               unsigned long long* __restrict__ map64 ) {
  const uint32_t tile  = blockIdx.x;
  const PatchDev pd    = patches[tilePatch[tile]];
  const int      local = int( tile ) - pd.blockBase;
  const int      u = ( local % pd.sizeU0 ) * occRes + int( threadIdx.x ) % occRes;
  const int      v = ( local / pd.sizeU0 ) * occRes + int( threadIdx.x ) / occRes;
  if ( u < pd.sizeU && v < pd.sizeV )
    map64[size_t( pd.depthOff - roundDepthBase ) + size_t( v ) * pd.sizeU + u] = pd.mode == 0 ? ~0ull : 0ull;
}

// one 16x16 tile (occupancy block) per workgroup: block peak, outlier filter, D0/D1 seed, source point id
__global__ __launch_bounds__( 256 ) void patchFilterTileKernel( const PatchDev* __restrict__ patches,
                                                                 const uint32_t* __restrict__ tilePatch,
                                                                 const unsigned long long* __restrict__ map64,
                                                                 int64_t roundDepthBase, int occRes, int surfaceThickness,
                                                                 int maxAllowedDepth, int32_t* __restrict__ d0tmp,
                                                                 int32_t* __restrict__ d1tmp, uint32_t* __restrict__ d0src ) {
  __shared__ int  wavePeak[4];
  const uint32_t  tile = blockIdx.x;
  const uint32_t  p    = tilePatch[tile];
  const PatchDev  pd   = patches[p];
  const int       local = int( tile ) - pd.blockBase;
  const int       bu = local % pd.sizeU0, bv = local / pd.sizeU0;
  const int       u = bu * occRes + int( threadIdx.x ) % occRes, v = bv * occRes + int( threadIdx.x ) / occRes;
  const bool      inside = u < pd.sizeU && v < pd.sizeV;
  const size_t    px     = size_t( pd.depthOff - roundDepthBase ) + size_t( v ) * pd.sizeU + u;
  const int       INF    = 32767;
  int             depth  = INF;
  uint32_t        src    = 0xFFFFFFFFu;
  if ( inside ) {
    const unsigned long long m = map64[px];
    const bool               empty = pd.mode == 0 ? ( m == ~0ull ) : ( m == 0ull );
    if ( !empty ) {
      depth = int( m >> 32 ) - 1;
      src   = uint32_t( m );
    }
  }
  // block peak: min depth (mode 0) or max depth (mode 1) over valid pixels
  int pk = depth == INF ? ( pd.mode == 0 ? INF : 0 ) : depth;
  pk = waveReduce( pk, [&]( int a, int b ) { return pd.mode == 0 ? min( a, b ) : max( a, b ); } );
  if ( ( threadIdx.x & 63 ) == 0 ) wavePeak[threadIdx.x >> 6] = pk;
  __syncthreads();
  pk = wavePeak[0];
#pragma unroll
  for ( int w = 1; w < 4; ++w ) pk = pd.mode == 0 ? min( pk, wavePeak[w] ) : max( pk, wavePeak[w] );
  if ( !inside ) return;
  if ( depth != INF ) {
    const int     dir = 1 - 2 * pd.mode;
    const int16_t a   = int16_t( abs( depth - pk ) );
    const int16_t b   = int16_t( int16_t( surfaceThickness ) + dir * depth );
    const int16_t c   = int16_t( dir * pd.d1 + int16_t( maxAllowedDepth ) );
    if ( a > 32 || b > c ) {
      depth = INF;
      src   = 0xFFFFFFFFu;
    }
  }
  d0tmp[px] = depth;
  d1tmp[px] = depth;
  d0src[px] = src;
}

// D1: farthest same-pixel depth within surfaceThickness of D0, colour-similar to the D0 point
template <bool LIST>
__global__ __launch_bounds__( 256 ) void patchDepth1Kernel( const Pt* __restrict__ pts, const uint8_t* __restrict__ rgb4,
                                                             const int32_t* __restrict__ pointPatch,
                                                             const PatchDev* __restrict__ patches, const uint32_t* __restrict__ list,
                                                             uint32_t count, uint32_t n, int64_t roundDepthBase, int surfaceThickness,
                                                             const int32_t* __restrict__ d0tmp,
                                                             const uint32_t* __restrict__ d0src, int32_t* __restrict__ d1tmp ) {
  const uint32_t i = roundPoint<LIST>( list, count, n );
  if ( i >= n ) return;
  const int32_t p = pointPatch[i];
  if ( p < 0 ) return;
  const PatchDev pd = patches[p];
  const Pt       q  = pts[i];
  const int      d = coordOf( q, pd.axN ), u = coordOf( q, pd.axT ) - pd.u1, v = coordOf( q, pd.axB ) - pd.v1;
  const size_t   px = size_t( pd.depthOff - roundDepthBase ) + size_t( v ) * pd.sizeU + u;
  const int      z0 = d0tmp[px];
  if ( !( z0 < 32767 ) ) return;
  const int     dir   = 1 - 2 * pd.mode;
  const int16_t delta = int16_t( dir * ( d - z0 ) );
  if ( !( delta <= int16_t( surfaceThickness ) && delta >= 0 ) ) return;
  const uchar4 ci = reinterpret_cast<const uchar4*>( rgb4 )[i];
  const uchar4 c0 = reinterpret_cast<const uchar4*>( rgb4 )[d0src[px]];
  if ( !( abs( int( c0.x ) - int( ci.x ) ) < 128 && abs( int( c0.y ) - int( ci.y ) ) < 128 &&
          abs( int( c0.z ) - int( ci.z ) ) < 128 ) )
    return;
  if ( pd.mode == 0 )
    atomicMax( &d1tmp[px], d );
  else
    atomicMin( &d1tmp[px], d );
}

// per tile: block occupancy, patch-local depths into the frame pools, resampled voxels into the bitmap,
// per-patch sizeD (max local depth) and d0Count
__global__ __launch_bounds__( 256 ) void patchResampleTileKernel( const PatchDev* __restrict__ patches,
                                                                   const uint32_t* __restrict__ tilePatch,
                                                                   int64_t roundDepthBase, int occRes,
                                                                   const int32_t* __restrict__ d0tmp,
                                                                   const int32_t* __restrict__ d1tmp, int bitmapBits,
                                                                   uint32_t* __restrict__ bitmap,
                                                                   int16_t* __restrict__ depth0, int16_t* __restrict__ depth1,
                                                                   uint8_t* __restrict__ occupancy,
                                                                   int32_t* __restrict__ patchStat /* [p][2] sizeD, d0Count */ ) {
  __shared__ int  anyValid[4], tileMax[4];
  const uint32_t  tile = blockIdx.x;
  const uint32_t  p    = tilePatch[tile];
  const PatchDev  pd   = patches[p];
  const int       local = int( tile ) - pd.blockBase;
  const int       bu = local % pd.sizeU0, bv = local / pd.sizeU0;
  const int       u = bu * occRes + int( threadIdx.x ) % occRes, v = bv * occRes + int( threadIdx.x ) / occRes;
  const bool      inside = u < pd.sizeU && v < pd.sizeV;
  bool            valid  = false;
  int             l0 = 0, l1 = 0;
  if ( inside ) {
    const size_t px = size_t( pd.depthOff - roundDepthBase ) + size_t( v ) * pd.sizeU + u;
    const int    z0 = d0tmp[px], z1 = d1tmp[px];
    int16_t      o0 = 32767, o1 = 32767;
    if ( z0 < 32767 ) {
      valid         = true;
      const int dir = 1 - 2 * pd.mode;
      l0            = dir * ( z0 - pd.d1 );
      l1            = dir * ( z1 - pd.d1 );
      o0            = int16_t( l0 );
      o1            = int16_t( l1 );
      // resampled points (D0 and D1) -> bitmap
      int c[3];
      c[pd.axT] = u + pd.u1;
      c[pd.axB] = v + pd.v1;
      c[pd.axN] = z0;
      size_t bit = size_t( c[0] ) + ( size_t( c[1] ) << bitmapBits ) + ( size_t( c[2] ) << ( 2 * bitmapBits ) );
      atomicOr( &bitmap[bit >> 5], 1u << ( bit & 31 ) );
      if ( z1 != z0 ) {
        c[pd.axN] = z1;
        bit       = size_t( c[0] ) + ( size_t( c[1] ) << bitmapBits ) + ( size_t( c[2] ) << ( 2 * bitmapBits ) );
        atomicOr( &bitmap[bit >> 5], 1u << ( bit & 31 ) );
      }
    }
    depth0[size_t( pd.depthOff ) + size_t( v ) * pd.sizeU + u] = o0;
    depth1[size_t( pd.depthOff ) + size_t( v ) * pd.sizeU + u] = o1;
  }
  // reductions over the tile
  const unsigned long long m  = __ballot( valid );
  const int                mx = waveMax( valid ? max( l0, l1 ) : 0 );
  // (one report per TILE -- rounds 1-5: one per wavefront -- and the maximum only if it can raise the patch's: a big patch is
  //  thousands of tiles adding to the same two words, ~ 11 ns each, one after the other; the look is a possibly stale view of a
  //  word that only grows)
  if ( ( threadIdx.x & 63 ) == 0 ) {
    anyValid[threadIdx.x >> 6] = __popcll( m );
    tileMax[threadIdx.x >> 6]  = mx;
  }
  __syncthreads();
  if ( threadIdx.x == 0 ) {
    const int count = anyValid[0] + anyValid[1] + anyValid[2] + anyValid[3];
    occupancy[size_t( pd.occOff ) + size_t( bv ) * pd.sizeU0 + bu] = count ? 1 : 0;
    if ( count ) {
      const int tmx = max( max( tileMax[0], tileMax[1] ), max( tileMax[2], tileMax[3] ) );
      if ( tmx > loadStaleOk( &patchStat[2 * p] ) ) atomicMax( &patchStat[2 * p], tmx );
      atomicAdd( &patchStat[2 * p + 1], count );
    }
  }
}

// ---- S9 -------------------------------------------------------------------------------------------------
// B probes of the voxel bitmap in one trip: offsets[o .. o + B) (FULL: all below nOffsets; else those beyond it repeat the last
// and count as no hit), d2 of the first hit in index order or kFar.  o is uniform: the offsets are one scalar load and what they
// add to a bit index is scalar arithmetic.  A cell outside the grid reads the word of `home` -- the point's own cell, clamped into
// the grid: an address the walk has read -- and counts as no hit.
constexpr int kProbeBatch = 8;
template <int B, bool FULL>
__device__ __forceinline__ uint32_t probeBatch( const uint32_t* __restrict__ bitmap, int bitmapBits, const int* __restrict__ offsets, int o,
                                                int nOffsets, const Pt q, size_t home ) {
  const uint32_t size = 1u << bitmapBits;
  int            packed[B];
#pragma unroll
  for ( int k = 0; k < B; ++k ) packed[k] = offsets[FULL ? o + k : min( o + k, nOffsets - 1 )];
  uint32_t word[B], hitBit[B];
#pragma unroll
  for ( int k = 0; k < B; ++k ) {
    const int dx = ( packed[k] & 0xFF ) - 128, dy = ( ( packed[k] >> 8 ) & 0xFF ) - 128, dz = ( ( packed[k] >> 16 ) & 0xFF ) - 128;
    const long long step = (long long)dx + ( (long long)dy << bitmapBits ) + ( (long long)dz << ( 2 * bitmapBits ) );
    const bool inside = uint32_t( q.x + dx ) < size && uint32_t( q.y + dy ) < size && uint32_t( q.z + dz ) < size &&
                        uint32_t( q.x ) < size && uint32_t( q.y ) < size && uint32_t( q.z ) < size && ( FULL || o + k < nOffsets );
    const size_t bit = inside ? size_t( (long long)home + step ) : home;
    hitBit[k]        = inside ? 1u << ( bit & 31 ) : 0u;
    word[k]          = bitmap[bit >> 5];
  }
  pinAll( word );
  uint32_t best = kFar;
#pragma unroll
  for ( int k = B - 1; k >= 0; --k )
    if ( word[k] & hitBit[k] ) best = uint32_t( packed[k] >> 24 );
  return best;
}

// dist2 of every point still raw to the resampled cloud, exact up to the probe radius, kFar beyond it.  A point that has come
// within thrSelection is raw no longer and never will be again (the bitmap only gains bits), and its dist is not read again: later
// rounds probe the points of the list alone.  keep[j] = the j-th point of the pass stays raw (the next list: rawListScatterKernel).
template <bool LIST>
__global__ __launch_bounds__( 256 ) void rawDistanceKernel( const Pt* __restrict__ pts, const uint32_t* __restrict__ list, uint32_t count,
                                                             const uint32_t* __restrict__ bitmap, int bitmapBits,
                                                             const int* __restrict__ offsets, int nOffsets,
                                                             uint32_t thrSelection, uint32_t* __restrict__ dist,
                                                             uint8_t* __restrict__ raw, uint32_t* __restrict__ keep ) {
  const uint32_t j = chunkedIndex();
  if ( j >= count ) return;
  const uint32_t i    = LIST ? list[j] : j;
  const Pt       q    = pts[i];
  // The first trip is the single probe of offset 0 (the point's own voxel): most points of round 1 have just been resampled and
  // end there -- a batch of speculative reads of a 128 MiB bitmap for each of them would be new HBM traffic.
  const int    top  = ( 1 << bitmapBits ) - 1;
  const size_t home = size_t( min( max( int( q.x ), 0 ), top ) ) + ( size_t( min( max( int( q.y ), 0 ), top ) ) << bitmapBits ) +
                      ( size_t( min( max( int( q.z ), 0 ), top ) ) << ( 2 * bitmapBits ) );
  uint32_t best = probeBatch<1, true>( bitmap, bitmapBits, offsets, 0, nOffsets, q, home );
  // Lanes still searching: kProbeBatch offsets in one uniform load, their bitmap words issued together, the hit of lowest index
  // wins -- offsets are sorted by d2 and carry it in the top byte, so this is the hit the probe-by-probe walk stopped at.  The
  // last, partial batch starts at an index every lane knows (a lane's own loop counter differs from lane to lane behind the loop).
  const int tail = 1 + ( nOffsets - 1 ) / kProbeBatch * kProbeBatch;
  for ( int o = 1; best == kFar && o < tail; o += kProbeBatch )
    best = probeBatch<kProbeBatch, true>( bitmap, bitmapBits, offsets, o, nOffsets, q, home );
  if ( best == kFar && tail < nOffsets ) best = probeBatch<kProbeBatch, false>( bitmap, bitmapBits, offsets, tail, nOffsets, q, home );
  const bool isRaw = best > thrSelection;
  dist[i]          = best;
  raw[i]           = isRaw ? 1 : 0;
  keep[j]          = isRaw ? 1u : 0u;
}

// The next round's list: the points that stay raw, in the order of this pass -- ascending, since the compaction is stable (pos = the
// exclusive scan of keep, whose total is the new count); posOf[i] = where the list holds point i.
template <bool LIST>
__global__ __launch_bounds__( 256 ) void rawListScatterKernel( const uint32_t* __restrict__ list, uint32_t count,
                                                                const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                                                                uint32_t* __restrict__ next, uint32_t* __restrict__ posOf ) {
  const uint32_t j = chunkedIndex();
  if ( j >= count || !keep[j] ) return;
  const uint32_t i = LIST ? list[j] : j;
  next[pos[j]]     = i;
  posOf[i]         = pos[j];
}

}  // namespace

// bit j of mutual[i] = knn[i][j] lists i in its own row.  Depends only on the adjacency: once per frame.
int ensureMutualMask( tmc2_frame* f ) {
  if ( f->haveMutual ) return TMC2_OK;
  const uint32_t n = uint32_t( f->n );
  TMC2_TRY( f->d_mutual.alloc( n ) );
  StageScope stage( f->ctx, "k:ccMutualMask" );
  // option MUTUAL_ORDER (this pass and S7's union / relaxation passes): "input" = index order, blocks as they come (rounds 1-5);
  // "chunk" = index order, XCD x on the x-th eighth of the blocks; "tree" = tree order, same eighths
  const PassOrder order  = passOrder( f, "MUTUAL_ORDER" );
  const uint32_t  blocks = ( n + 255 ) / 256;
  hipLaunchKernelGGL( ccMutualMaskKernel<16>, dim3( order.chunked ? chunkedGrid( blocks ) : blocks ), dim3( 256 ), 0, f->ctx->stream, f->d_knn.p,
                      order.perm, order.chunked, n, f->d_mutual.p );
  TMC2_HIP( hipGetLastError() );
  f->haveMutual = true;
  return TMC2_OK;
}

int segmentPatches( tmc2_frame* f, const tmc2_segmenter_params* sp ) {
  if ( !f->haveKnn || !f->havePartition ) {
    setError( "segmentPatches: adjacency / partition missing" );
    return TMC2_E_STATE;
  }
  if ( f->k != sp->maxNNCountPatchSegmentation || f->k != 16 ) {
    setError( "segmentPatches: maxNNCountPatchSegmentation=%d must equal the resident adjacency k=%d (16)",
              sp->maxNNCountPatchSegmentation, f->k );
    return TMC2_E_UNSUPPORTED;
  }
  if ( f->d_rgb.count == 0 ) {
    setError( "segmentPatches: the frame has no colours (needed by the D1 colour-similarity test)" );
    return TMC2_E_STATE;
  }
  if ( sp->occupancyResolution != 16 ) {
    setError( "segmentPatches: occupancyResolution=%d unsupported (tiles are 16x16)", sp->occupancyResolution );
    return TMC2_E_UNSUPPORTED;
  }
  tmc2_ctx*      ctx = f->ctx;
  hipStream_t    s   = ctx->stream;
  const uint32_t n   = uint32_t( f->n );
  const int      occRes = sp->occupancyResolution;
  const uint32_t thrDet = uint32_t( std::floor( sp->maxAllowedDist2RawPointsDetection ) );
  const uint32_t thrSel = uint32_t( std::floor( sp->maxAllowedDist2RawPointsSelection ) );
  const int      probeR2 = int( std::max( thrDet, thrSel ) );
  if ( probeR2 > 27 ) {
    setError( "segmentPatches: raw-point distance thresholds above 27 unsupported" );
    return TMC2_E_UNSUPPORTED;
  }
  // probe offsets sorted by d2 (d2 in the top byte)
  std::vector<int> offsets;
  {
    int R = 0;
    while ( R * R <= probeR2 ) ++R;
    std::vector<std::pair<int, int>> tmp;
    for ( int dz = -R; dz <= R; ++dz )
      for ( int dy = -R; dy <= R; ++dy )
        for ( int dx = -R; dx <= R; ++dx ) {
          const int d2 = dx * dx + dy * dy + dz * dz;
          if ( d2 <= probeR2 ) tmp.emplace_back( d2, ( dx + 128 ) | ( ( dy + 128 ) << 8 ) | ( ( dz + 128 ) << 16 ) );
        }
    std::sort( tmp.begin(), tmp.end() );
    for ( auto& t : tmp ) offsets.push_back( t.second | ( t.first << 24 ) );
  }
  int bitmapBits = 1;
  while ( ( 1 << bitmapBits ) <= int( f->geoMax ) ) ++bitmapBits;
  const size_t bitmapWords = ( size_t( 1 ) << ( 3 * bitmapBits ) ) >> 5;
  TMC2_TRY( ctx->voxelBitmap.alloc( bitmapWords ) );

  DevBuf<uint32_t> d_label, d_ccCount, d_flag, d_rank, d_dist, d_small, d_d0src, d_parent, d_root, d_lab, d_rawList[2], d_posOf;
  DevBuf<uint8_t>  d_raw, d_tables;
  DevBuf<int32_t>  d_pointPatch, d_minUv, d_bbox, d_patchStat, d_d0tmp, d_d1tmp;
  DevBuf<unsigned long long> d_map64;
  TMC2_TRY( d_label.alloc( n ) );
  TMC2_TRY( d_parent.alloc( n ) );
  TMC2_TRY( d_root.alloc( n ) );
  TMC2_TRY( d_lab.alloc( n ) );
  TMC2_TRY( d_ccCount.alloc( n ) );
  TMC2_TRY( d_flag.alloc( n ) );
  TMC2_TRY( d_rank.alloc( n ) );
  TMC2_TRY( d_dist.alloc( n ) );
  TMC2_TRY( d_raw.alloc( n ) );
  TMC2_TRY( d_pointPatch.alloc( n ) );
  TMC2_TRY( d_rawList[0].alloc( n ) );
  TMC2_TRY( d_rawList[1].alloc( n ) );
  TMC2_TRY( d_posOf.alloc( n ) );
  TMC2_TRY( d_small.alloc( 16 ) );
  const int* d_offsets = ctx->constTable( ( uint64_t( 0x5339 ) << 32 ) | uint64_t( probeR2 ), offsets );  // (S9's probe offsets: a function of the thresholds)
  if ( !d_offsets ) return TMC2_E_HIP;
  TMC2_TRY( fillRegions( ctx, {{ctx->voxelBitmap.p, bitmapWords * 4, 0},
                               {d_raw.p, n, 1},
                               {d_dist.p, size_t( n ) * 4, 0xFF},
                               {d_small.p, 64, 0}} ) );

  f->patches.clear();
  f->patchesChanged();  // (a packing of the old list, and everything made from it, must not be read with the new one)
  f->depthCount = 0;
  f->occCount   = 0;
  // (the one-point-per-lane passes of S7-S9: XCD x takes the x-th eighth of the blocks -- chunkedIndex)
  const dim3  blk( 256 ), grdN( chunkedGrid( ( n + 255 ) / 256 ) );
  uint32_t    rawCount = n, relaxToken = 0;
  int        rounds   = 0;
  TMC2_TRY( ensureMutualMask( f ) );  // usually there already: the orientation (S3) needs the same bits
  DevBuf<uint16_t>& d_mutual   = f->d_mutual;
  const bool        agentScope = unionAgentScope( f->ctx );
  // the union / relaxation passes of round 1: option MUTUAL_ORDER as in ensureMutualMask (grdN is a multiple of 8 blocks either way)
  const PassOrder order   = passOrder( f, "MUTUAL_ORDER" );
  const bool      chunked = order.chunked;
  const uint32_t* perm    = order.perm;
  const uint32_t  minCount = uint32_t( sp->minPointCountPerCCPatchSegmentation );
  // Round 1 runs every per-point pass over all n points: every one is raw.  Each round's raw-point update leaves the list of the points
  // still raw (ascending) and their number, and the per-point passes of the later rounds run over that list (roundPoint).  What the
  // n-wide form of a pass wrote for a point that is not raw -- lab / ccCount / parent (ccInit), label = kNoLabel (ccLabelCount), flag = 0
  // (ccSeedFlag), pointPatch = -1 (ccAssign), dist and raw = 0 (rawDistance) -- is read by nobody: every per-point pass starts from
  // a listed point; lab, root, ccCount and rank are looked up at roots, labels and seeds, which are raw points of this round;
  // knn rows lead to other points only behind the test of raw[v], which rawDistance brings to 0 once; the tile passes read the depth
  // maps, never a per-point array; and d_label, d_pointPatch, d_dist and d_raw do not outlive this call.
  // ROUND_KERNEL: the instance of a per-point kernel this round launches (one body each, the index source a template argument)
#define ROUND_KERNEL( name, ... ) ( listed ? name<true, ##__VA_ARGS__> : name<false, ##__VA_ARGS__> )
  bool listed = false;
  int  cur    = 0;  // d_rawList[cur]: this round's list (from round 2 on)
  // A component needs minPointCountPerCCPatchSegmentation points to become a patch (reference :833), and a round without one ends
  // the reference's loop (:900) with the patches made so far: with fewer points than that left raw the round is not queued at all.
  while ( rawCount > 0 && rawCount >= minCount ) {
    const uint32_t* list  = listed ? d_rawList[cur].p : nullptr;
    const uint32_t  count = rawCount;  // (round 1: n)
    const dim3      grd   = listed ? dim3( chunkedGrid( ( count + 255 ) / 256 ) ) : grdN;
    // ---- S7 -----------------------------------------------------------------------------------------
    StageScope cc( ctx, "patches_cc" );
    hipLaunchKernelGGL( ROUND_KERNEL( ccInitKernel, 16 ), grd, blk, 0, s, f->d_knn.p, d_mutual.p, f->d_partition.p, d_raw.p, perm, chunked,
                        list, count, n, d_parent.p, d_lab.p, d_ccCount.p );
    {
      StageScope kt( ctx, "k:ccUnion" );
      hipLaunchKernelGGL( ROUND_KERNEL( ccUnionKernel, 16 ), grd, blk, 0, s, f->d_knn.p, d_mutual.p, f->d_partition.p, d_raw.p, perm,
                          chunked, list, count, n, d_parent.p, unionPrecheck( f->ctx ), agentScope );
      kt.end();
      if ( unionCheck( f->ctx ) ) {  // debug invariants (soak tests): costs a round trip
        TMC2_HIP( hipMemsetAsync( d_small.p + 8, 0, 8, s ) );
        hipLaunchKernelGGL( ROUND_KERNEL( ccCheckKernel, 16 ), grd, blk, 0, s, f->d_knn.p, d_mutual.p, f->d_partition.p, d_raw.p, list,
                            count, n, d_parent.p, d_small.p + 8 );
        TMC2_TRY( unionCheckResult( s, d_small.p + 8, "segmentPatches: union-find invariant broken in round " + std::to_string( rounds ) ) );
      }
      hipLaunchKernelGGL( ROUND_KERNEL( ccFlattenSeedKernel ), grd, blk, 0, s, d_raw.p, d_dist.p, thrDet, list, count, n, d_parent.p,
                          d_root.p, d_lab.p, agentScope );
    }
    // a few sweeps, then -- speculatively -- the labelling and the seed count, and ONE round trip for both answers: "did the
    // last sweep of the batch still change a label" (then sweep on and label again) and the number of patches
    uint32_t P = 0;
    for ( int guard = 0; guard < 1 << 20; ++guard ) {
      StageScope kt( ctx, "k:ccRelax" );
      for ( int b = 0; b < 3; ++b )
        hipLaunchKernelGGL( ROUND_KERNEL( ccRelaxKernel, 16 ), grd, blk, 0, s, f->d_knn.p, d_mutual.p, f->d_partition.p, d_raw.p,
                            d_root.p, perm, chunked, list, count, n, d_lab.p, d_small.p, ++relaxToken, agentScope );
      kt.end();
      hipLaunchKernelGGL( ROUND_KERNEL( ccLabelCountKernel ), grd, blk, 0, s, d_raw.p, d_root.p, d_lab.p, list, count, n, minCount,
                          d_label.p, d_ccCount.p );
      hipLaunchKernelGGL( ROUND_KERNEL( ccSeedFlagKernel ), grd, blk, 0, s, d_label.p, d_ccCount.p, minCount, list, count, d_flag.p );
      // (both answers in the context's page-locked line, stored by the scan's last tile: [0] the number of patches, [1] the token of
      //  the last sweep that changed a label -- no copy)
      volatile uint32_t* answer = ctx->answerLine( tmc2_ctx::kAnswerPatchRound );
      TMC2_TRY( exclusiveScanU32( ctx, d_flag.p, d_rank.p, count, d_small.p + 1, ScanAnswer{answer, d_small.p, 1} ) );
      TMC2_HIP( hipStreamSynchronize( s ) );
      P = answer[0];
      if ( answer[1] != relaxToken ) break;
      // (ccCount is an accumulation: start it over before labelling again)
      if ( listed )
        hipLaunchKernelGGL( ccClearCountKernel, grd, blk, 0, s, list, count, d_ccCount.p );
      else
        TMC2_HIP( hipMemsetAsync( d_ccCount.p, 0, size_t( n ) * 4, s ) );
    }
    cc.end();
    if ( P == 0 ) break;
    // ---- S8 -----------------------------------------------------------------------------------------
    StageScope build( ctx, "patches_build" );
    TMC2_TRY( d_minUv.alloc( 2 * size_t( P ) ) );
    TMC2_TRY( d_bbox.alloc( 7 * size_t( P ) ) );           // boxes, then the views: one copy to the host
    const size_t statWords = 2 * size_t( P );
    TMC2_TRY( d_patchStat.alloc( statWords ) );
    int32_t* d_view = d_bbox.p + 6 * size_t( P );
    hipLaunchKernelGGL( ROUND_KERNEL( ccAssignKernel ), grd, blk, 0, s, d_label.p, d_ccCount.p, d_rank.p, d_posOf.p, f->d_partition.p,
                        minCount, list, count, n, d_pointPatch.p, d_view );
    hipLaunchKernelGGL( patchBoundsInitKernel, dim3( ( P + 255 ) / 256 ), blk, 0, s, P, d_bbox.p, d_minUv.p, d_patchStat.p );
    if ( sp->enablePatchSplitting )
      hipLaunchKernelGGL( ROUND_KERNEL( patchMinUvKernel ), grd, blk, 0, s, f->d_pts.p, d_pointPatch.p, d_view, list, count, n,
                          d_minUv.p );
    hipLaunchKernelGGL( ROUND_KERNEL( patchTrimBboxKernel ), grd, blk, 0, s, f->d_pts.p, d_view, d_minUv.p, sp->enablePatchSplitting,
                        sp->maxPatchSize, list, count, n, d_pointPatch.p, d_bbox.p );
    // (boxes + views, and further down the counters, land in the context's page-locked staging: plain DMA, no staging copy behind it)
    int32_t* h_records = ctx->hostRecords.get<int32_t>( std::max<size_t>( 7 * size_t( P ) + statWords, size_t( 1 ) << 16 ) );
    if ( !h_records ) {
      setError( "segmentPatches: hipHostMalloc failed" );
      return TMC2_E_HIP;
    }
    const int32_t* h_bbox = h_records;
    TMC2_HIP( hipMemcpyAsync( h_records, d_bbox.p, 7 * size_t( P ) * 4, hipMemcpyDeviceToHost, s ) );
    const int32_t* h_view = h_bbox + 6 * size_t( P );
    TMC2_HIP( hipStreamSynchronize( s ) );
    // A component of which patch splitting kept no point (none lies within maxPatchSize of its (min u, min v) corner: an L, a
    // diagonal band) has no box.  The reference makes an empty patch of it, the component stays raw, and its loop over the raw
    // points repeats that round for ever: the call ends here, before a size is derived from a box that does not exist.
    for ( uint32_t p = 0; p < P; ++p )
      if ( h_bbox[6 * p] > h_bbox[6 * p + 3] ) {
        f->patches.clear();
        f->depthCount = f->occCount = 0;
        f->havePatches              = false;
        setError( "segmentPatches: patch splitting with maxPatchSize=%d keeps no point of a connected component (round %d); "
                  "the reference does not terminate on this input",
                  sp->maxPatchSize, rounds );
        return TMC2_E_UNSUPPORTED;
      }
    // patch geometry on the host (P is a few hundred): axes, sizes, depth origin, pool offsets, tile list
    static const int       AX[3][3] = {{0, 2, 1}, {1, 2, 0}, {2, 0, 1}};
    std::vector<PatchDev>  h_pdLocal( P );
    PatchDev*              h_pd           = h_pdLocal.data();
    size_t                 tilesSoFar     = 0;
    const size_t           patchBase      = f->patches.size();
    const int64_t          roundDepthBase = f->depthCount;
    for ( uint32_t p = 0; p < P; ++p ) {
      tmc2_patch T{};
      T.index          = int32_t( patchBase + p );
      T.viewId         = h_view[p];
      const int* ax    = AX[T.viewId % 3];
      T.normalAxis     = ax[0];
      T.tangentAxis    = ax[1];
      T.bitangentAxis  = ax[2];
      T.projectionMode = T.viewId / 3;
      const int32_t* bb = &h_bbox[6 * p];
      T.u1    = bb[ax[1]];
      T.v1    = bb[ax[2]];
      T.sizeU = 1 + bb[3 + ax[1]] - bb[ax[1]];
      T.sizeV = 1 + bb[3 + ax[2]] - bb[ax[2]];
      const int L = sp->minLevel;
      T.d1        = T.projectionMode == 0 ? ( bb[ax[0]] / L ) * L
                                          : int( std::ceil( double( bb[3 + ax[0]] ) / double( L ) ) ) * L;
      T.sizeU0    = ( T.sizeU - 1 ) / occRes + 1;
      T.sizeV0    = ( T.sizeV - 1 ) / occRes + 1;
      T.size2DXInPixel = T.sizeU;
      T.size2DYInPixel = T.sizeV;
      if ( sp->quantizerSizeX )
        T.size2DXInPixel = int( std::ceil( double( T.sizeU ) / double( sp->quantizerSizeX ) ) * sp->quantizerSizeX );
      if ( sp->quantizerSizeY )
        T.size2DYInPixel = int( std::ceil( double( T.sizeV ) / double( sp->quantizerSizeY ) ) * sp->quantizerSizeY );
      T.depthOffset = f->depthCount;
      T.occOffset   = f->occCount;
      f->depthCount += int64_t( T.sizeU ) * T.sizeV;
      f->occCount += int64_t( T.sizeU0 ) * T.sizeV0;
      PatchDev& D = h_pd[p];
      D.u1 = T.u1, D.v1 = T.v1, D.d1 = T.d1;
      D.sizeU = T.sizeU, D.sizeV = T.sizeV, D.sizeU0 = T.sizeU0, D.sizeV0 = T.sizeV0;
      D.axN = ax[0], D.axT = ax[1], D.axB = ax[2], D.mode = T.projectionMode;
      D.blockBase = int32_t( tilesSoFar );
      D.depthOff  = T.depthOffset;
      D.occOff    = T.occOffset;
      tilesSoFar += size_t( T.sizeU0 ) * T.sizeV0;
      f->patches.push_back( T );
    }
    const size_t roundArea = size_t( f->depthCount - roundDepthBase );
    const uint32_t tiles   = uint32_t( tilesSoFar );
    // the round's two tables in the context's page-locked staging (patch records | tile -> patch): the copies below are DMA from it;
    // the round's last synchronisation (the counters) comes before the next round refills it
    const size_t pdBytes = ( size_t( P ) * sizeof( PatchDev ) + 15 ) & ~size_t( 15 );
    uint8_t*     h_tables = ctx->hostTables.get<uint8_t>( std::max<size_t>( pdBytes + size_t( tiles ) * 4, size_t( 1 ) << 20 ) );
    if ( !h_tables ) {
      setError( "segmentPatches: hipHostMalloc failed" );
      return TMC2_E_HIP;
    }
    memcpy( h_tables, h_pd, size_t( P ) * sizeof( PatchDev ) );
    uint32_t* h_tilePatch = reinterpret_cast<uint32_t*>( h_tables + pdBytes );
    for ( uint32_t p = 0, at = 0; p < P; ++p )
      for ( uint32_t b = uint32_t( h_pd[p].sizeU0 ) * uint32_t( h_pd[p].sizeV0 ); b > 0; --b ) h_tilePatch[at++] = p;
    TMC2_TRY( f->growPools() );
    TMC2_TRY( d_map64.alloc( roundArea ) );
    TMC2_TRY( d_d0tmp.alloc( roundArea ) );
    TMC2_TRY( d_d1tmp.alloc( roundArea ) );
    TMC2_TRY( d_d0src.alloc( roundArea ) );
    // (both tables in one allocation, as they lie in the staging: one copy)
    TMC2_TRY( d_tables.alloc( pdBytes + size_t( tiles ) * 4 ) );
    const PatchDev* d_patches   = reinterpret_cast<const PatchDev*>( d_tables.p );
    const uint32_t* d_tilePatch = reinterpret_cast<const uint32_t*>( d_tables.p + pdBytes );
    TMC2_HIP( hipMemcpyAsync( d_tables.p, h_tables, pdBytes + size_t( tiles ) * 4, hipMemcpyHostToDevice, s ) );
    hipLaunchKernelGGL( patchInitTileKernel, dim3( tiles ), blk, 0, s, d_patches, d_tilePatch, roundDepthBase, occRes, d_map64.p );
    hipLaunchKernelGGL( ROUND_KERNEL( patchDepth0Kernel ), grd, blk, 0, s, f->d_pts.p, d_pointPatch.p, d_patches, list, count, n,
                        roundDepthBase, d_map64.p );
    hipLaunchKernelGGL( patchFilterTileKernel, dim3( tiles ), blk, 0, s, d_patches, d_tilePatch, d_map64.p, roundDepthBase, occRes,
                        sp->surfaceThickness, sp->maxAllowedDepth, d_d0tmp.p, d_d1tmp.p, d_d0src.p );
    if ( sp->surfaceThickness > 0 )
      hipLaunchKernelGGL( ROUND_KERNEL( patchDepth1Kernel ), grd, blk, 0, s, f->d_pts.p, f->d_rgb.p, d_pointPatch.p, d_patches, list,
                          count, n, roundDepthBase, sp->surfaceThickness, d_d0tmp.p, d_d0src.p, d_d1tmp.p );
    hipLaunchKernelGGL( patchResampleTileKernel, dim3( tiles ), blk, 0, s, d_patches, d_tilePatch, roundDepthBase, occRes, d_d0tmp.p,
                        d_d1tmp.p, bitmapBits, ctx->voxelBitmap.p, f->d_depth0.p, f->d_depth1.p, f->d_occupancy.p, d_patchStat.p );
    int32_t* h_stat = h_records + 7 * size_t( P );
    // ---- S9 -----------------------------------------------------------------------------------------
    // the points that stay raw, compacted (stable: ascending) into the next round's list; their number comes back in the answer line,
    // whose content of this round (the number of patches, the sweep token) has been read
    volatile uint32_t* answer = ctx->answerLine( tmc2_ctx::kAnswerPatchRound );
    hipLaunchKernelGGL( ROUND_KERNEL( rawDistanceKernel ), grd, blk, 0, s, f->d_pts.p, list, count, ctx->voxelBitmap.p, bitmapBits,
                        d_offsets, int( offsets.size() ), thrSel, d_dist.p, d_raw.p, d_flag.p );
    const int scanned = exclusiveScanU32( ctx, d_flag.p, d_rank.p, count, nullptr, ScanAnswer{answer, nullptr, 0} );
    if ( scanned != TMC2_OK ) {
      (void)hipStreamSynchronize( s );  // (the copy from the staging above is queued: not left in flight)
      return scanned;
    }
    hipLaunchKernelGGL( ROUND_KERNEL( rawListScatterKernel ), grd, blk, 0, s, list, count, d_flag.p, d_rank.p, d_rawList[cur ^ 1].p,
                        d_posOf.p );
    TMC2_HIP( hipMemcpyAsync( h_stat, d_patchStat.p, statWords * 4, hipMemcpyDeviceToHost, s ) );
    TMC2_HIP( hipStreamSynchronize( s ) );
    const uint32_t rawBefore = rawCount;
    rawCount                 = answer[0];
    cur ^= 1;
    listed = true;
    build.end();
    // A pixel that passes the depth filter holds an input point that was raw and now lies on the resampled cloud, so a round with
    // one such pixel shortens the list.  A round that does not has changed nothing and would be repeated for ever (the
    // reference's loop is; tmc2_segmenter_params_check refuses the parameter range in which that can happen).
    if ( rawCount >= rawBefore ) {
      f->patches.clear();
      f->depthCount = f->occCount = 0;
      f->havePatches              = false;
      setError( "segmentPatches: round %d took no point off the raw list (%u left); the reference does not terminate on this input",
                rounds, rawCount );
      return TMC2_E_UNSUPPORTED;
    }
    for ( uint32_t p = 0; p < P; ++p ) {
      tmc2_patch& T = f->patches[patchBase + p];
      const int   sizeD = h_stat[2 * p];
      T.sizeDPixel      = sizeD;
      const int bits    = std::min( sp->geometryBitDepth3D, sp->geometryBitDepth2D );
      const int L       = sp->minLevel;
      const int sd      = std::min( ( 1 << bits ) - 1, sizeD );
      const int bitsD   = bits - int( std::log2( L ) );
      int       q       = sd == 0 ? 0 : ( ( sd - 1 ) / L + 1 );
      q                 = std::min( q, ( 1 << bitsD ) - 1 );
      T.sizeD           = q == 0 ? 0 : ( q * L - 1 );
      T.d0Count         = h_stat[2 * p + 1];
      T.eomAndD1Count   = 0;
    }
    ++rounds;
  }
#undef ROUND_KERNEL
  TMC2_HIP( hipGetLastError() );
  f->rounds      = rounds;
  f->havePatches = true;
  f->geometryBitDepth3D = sp->geometryBitDepth3D;  // (the cube of T6's grid)
  return TMC2_OK;
}

}  // namespace tmc2

// S7's own kernels -- mutual mask, initial forest, union pass, the check, the find of the flatten pass -- on a neighbour table the
// caller supplies (selftest.hip: the primitives under test), with the launch shapes and the options (MUTUAL_ORDER, UF_PRECHECK,
// UF_SCOPE, UF_CHECK) of segmentPatches.  d_perm: the order "tree" walks (null: index order).  d_root[u] for raw points; d_bad[2] as
// ccCheckKernel counts (left alone without UF_CHECK).  Queued, not waited for.
extern "C" int tmc2_selftest_components( tmc2_ctx* ctx, const uint32_t* d_knn, const uint8_t* d_partition, const uint8_t* d_raw,
                                         const uint32_t* d_perm, uint64_t n64, uint32_t* d_root, uint32_t* d_bad ) {
  using namespace tmc2;
  if ( !ctx || !d_knn || !d_partition || !d_raw || !d_root || !d_bad || n64 == 0 || n64 > 0x0FFFFFFFull ) {
    setError( "selftest_components: invalid argument (null pointer, no point, or more than 2^28 - 1 points)" );
    return TMC2_E_INVALID;
  }
  ApiScope         scope( ctx );
  hipStream_t      s = ctx->stream;
  const uint32_t   n = uint32_t( n64 );
  DevBuf<uint16_t> d_mutual;
  DevBuf<uint32_t> d_parent, d_lab, d_ccCount, d_dist;
  TMC2_TRY( d_mutual.alloc( n ) );
  TMC2_TRY( d_parent.alloc( n ) );
  TMC2_TRY( d_lab.alloc( n ) );
  TMC2_TRY( d_ccCount.alloc( n ) );
  TMC2_TRY( d_dist.alloc( n ) );
  // (a point a pass skipped must show as a wrong root, not as a link read from what the pool handed out: every link starts at 0)
  TMC2_TRY( fillRegions( ctx, {{d_parent.p, size_t( n ) * 4, 0}, {d_mutual.p, size_t( n ) * 2, 0}, {d_dist.p, size_t( n ) * 4, 0}} ) );
  const auto      option  = ctxOption( ctx, "MUTUAL_ORDER" );
  const char      o       = option ? ( *option )[0] : 'c';
  const bool      chunked = o != 'i';
  const uint32_t* perm    = o == 't' ? d_perm : nullptr;
  const uint32_t  blocks  = ( n + 255 ) / 256;
  const dim3      blk( 256 ), grdN( chunkedGrid( blocks ) );
  const bool      agentScope = unionAgentScope( ctx );
  hipLaunchKernelGGL( ccMutualMaskKernel<16>, dim3( chunked ? chunkedGrid( blocks ) : blocks ), dim3( 256 ), 0, s, d_knn, perm, chunked, n,
                      d_mutual.p );
  // (the round-1 form of the passes: over all n points, no list)
  const uint32_t* noList = nullptr;
  hipLaunchKernelGGL( ( ccInitKernel<false, 16> ), grdN, blk, 0, s, d_knn, d_mutual.p, d_partition, d_raw, perm, chunked, noList, n, n,
                      d_parent.p, d_lab.p, d_ccCount.p );
  hipLaunchKernelGGL( ( ccUnionKernel<false, 16> ), grdN, blk, 0, s, d_knn, d_mutual.p, d_partition, d_raw, perm, chunked, noList, n, n,
                      d_parent.p, unionPrecheck( ctx ), agentScope );
  if ( unionCheck( ctx ) )
    hipLaunchKernelGGL( ( ccCheckKernel<false, 16> ), grdN, blk, 0, s, d_knn, d_mutual.p, d_partition, d_raw, noList, n, n, d_parent.p,
                        d_bad );
  // (no point is a seed: no distance exceeds the threshold)
  hipLaunchKernelGGL( ccFlattenSeedKernel<false>, grdN, blk, 0, s, d_raw, d_dist.p, 0xFFFFFFFFu, noList, n, n, d_parent.p, d_root,
                      d_lab.p, agentScope );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}
