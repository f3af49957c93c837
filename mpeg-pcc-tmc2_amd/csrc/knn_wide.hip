// knn_wide.hip -- exact nanoflann-order k-NN for result counts beyond the per-lane kernel's, on gfx950 (MI355X).
//
// Replaces PCCKdTree::search as PCCPatchSegmenter3::computeAdjacencyInfo calls it with maxNNCountRefineSegmentation results
// (PccLibEncoder/source/PCCPatchSegmenter.cpp:267-291; nanoflann searchLevel / KNNResultSet::addPoint, nanoflann.hpp:1207-1254,
// 110-131).  knn.hip keeps one query per lane and the k-best list in VGPRs: it ends at k = 32.  Here ONE WAVEFRONT takes one query:
//   * the walk is knnKernel's -- near-descend / far-stack, a far child visited iff mindist <= worst when it is popped, the cap of
//     the K-th distance from K tree-order neighbours before the first descent -- with wave-uniform state: node, offsets, the
//     pending far children on a stack of the wave's own in LDS;
//   * in a leaf the lanes take the points; the candidates below the current worst are then entered ONE BY ONE in tree order
//     (the reference's order of arrival decides between equal distances) into a distance-sorted list of K entries in LDS, spread
//     over the lanes: entries above the candidate move up by one, 64 per step from the top, until a step meets an entry <= the
//     candidate; ballot + popcount of that step give the slot "behind every entry <= d".  That IS the reference's tie rule,
//     with no visit number stored; a full list drops its last entry, and a candidate equal to the worst never gets here.
//   * LDS: 8 bytes x K of list + 1 KiB of stack per wave, four waves to a workgroup: 36 KiB at K = 1024, sized from K.
// The result is a SET: rows are written in list order, which callers must not rely on.  Queries run in tree order (the frame's
// own points) so that the waves of a workgroup, and the workgroups of an XCD (internal.h: the XCD work mapping), walk the same
// part of the tree.  Every loop is bounded: the descent by the tree's depth, the walk by its node count, the list steps by K / 64.
// Squared distances are 32-bit unsigned: every coordinate, of the tree and of the queries, must be >= -4096 (3 x 36863^2 < 2^32).
#include "internal.h"
#include "kd_walk.h"
#include "refine_knn.h"
#include "wave.h"

namespace tmc2 {
namespace {

constexpr int      kWideStack = 64;           // pending far children: at most one per level (dispatch checks the depth)
constexpr uint32_t kWideInf   = 0xFFFFFFFFu;  // worst of a list that is not full yet
constexpr int      kWideWaves = 4;            // queries per workgroup
constexpr int      kWideMinCoord = -4096;

// a word of the wave's LDS region: local address space spelled out (a generic volatile pointer is lowered to flat, system-coherent
// accesses), volatile because the lanes of a wave hand entries to each other through it, in program order
using LdsWord = volatile __attribute__( ( address_space( 3 ) ) ) uint32_t;

__device__ __forceinline__ uint32_t wideDist( int qx, int qy, int qz, Pt c ) {
  const int ex = qx - c.x, ey = qy - c.y, ez = qz - c.z;
  return uint32_t( ex * ex ) + uint32_t( ey * ey ) + uint32_t( ez * ez );
}

// candidate (d, p) into the wave's list; precondition d < worst.  Entries [at, top) move up by one, from the top, 64 per step (a
// step reads its 64 entries before it writes them one slot higher: the slots it writes belong to itself or to the step before)
__device__ __forceinline__ void wideInsert( LdsWord* ld, LdsWord* li, uint32_t K, uint32_t& count, uint32_t d, uint32_t p,
                                            uint32_t lane ) {
  const uint32_t top = min( count, K - 1u );  // (a full list drops entry K - 1)
  uint32_t       at  = 0;
  for ( int base = int( ( top + 63u ) & ~63u ) - 64; base >= 0; base -= 64 ) {
    const uint32_t e  = uint32_t( base ) + lane;
    const bool     in = e < top;
    const uint32_t v = in ? ld[e] : 0u, iv = in ? li[e] : 0u;
    const bool     up = in && v > d;
    const unsigned long long stay = __ballot( in && !up );
    __builtin_amdgcn_wave_barrier();
    if ( up ) ld[e + 1] = v, li[e + 1] = iv;
    __builtin_amdgcn_wave_barrier();
    if ( stay ) {  // (sorted: the entries <= d of this step are its lowest)
      at = uint32_t( base ) + uint32_t( __popcll( stay ) );
      break;
    }
  }
  if ( lane == 0 ) ld[at] = d, li[at] = p;
  __builtin_amdgcn_wave_barrier();
  count = min( count + 1u, K );
}

// queries == nullptr: the tree-order points themselves (query j = tree position j).
// TRANSPOSED = false: out[row][K] of ORIGINAL indices, row = perm[j] for the tree's own points, j for foreign queries
// TRANSPOSED = true : out[e * outStride + j] = TREE POSITION of result e of query j (the voting kernel's layout, refine_knn.hip)
template <bool TRANSPOSED>
__global__ __launch_bounds__( 64 * kWideWaves ) void knnWideKernel( const Pt* __restrict__ ptsTree, const uint32_t* __restrict__ perm,
                                                                    const KdNode* __restrict__ nodes, KdBox root, const Pt* __restrict__ queries,
                                                                    uint32_t nq, uint32_t nTree, uint32_t K, uint32_t nodeBudget,
                                                                    uint32_t* __restrict__ out, uint32_t outStride ) {
  extern __shared__ uint32_t wideLds[];  // per wave: dist[K] | position[K] | stack[kWideStack][4]
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t j = chunkedBlock( gridDim.x >> 3 ) * kWideWaves + wave;
  if ( j >= nq ) return;  // (the whole wave; no workgroup barrier anywhere below)
  LdsWord* ld = (LdsWord*)wideLds + wave * ( 2u * K + 4u * kWideStack );
  LdsWord* li = ld + K;
  LdsWord* st = li + K;
  for ( uint32_t e = lane; e < K; e += 64u ) ld[e] = kWideInf, li[e] = 0u;

  const Pt  qp = queries ? queries[j] : ptsTree[j];
  const int qx = qp.x, qy = qp.y, qz = qp.z;
  KdOffsets o  = kdInitialOffsets( root, qx, qy, qz );  // (the walk and its offsets: kd_walk.h)

  // the cap (knnKernel): K real points around the query in tree order bound the K-th distance from above; what lies beyond cannot
  // stay in the list, and skipping it leaves the order of arrival of everything else as it was
  uint32_t cap = 0;
  {
    uint32_t centre = j;
    if ( queries ) {
      KdNode nd = nodes[0];
      for ( int level = 0; nd.dim >= 0 && level < kWideStack; ++level ) nd = nodes[kdNearChild( nd, qx, qy, qz )];
      centre = nd.dim < 0 ? uint32_t( nd.a + nd.b ) >> 1 : 0u;
    }
    const uint32_t first = min( centre > K / 2u ? centre - K / 2u : 0u, nTree - K );
    for ( uint32_t e = lane; e < K; e += 64u ) cap = max( cap, wideDist( qx, qy, qz, ptsTree[first + e] ) );
    cap = waveMax( cap );
  }
  __builtin_amdgcn_wave_barrier();

  uint32_t count = 0, worst = kWideInf, sp = 0, node = 0, visits = 0;
  for ( ;; ) {
    KdNode nd = nodes[node];
    for ( int level = 0; nd.dim >= 0 && level <= kWideStack; ++level ) {
      const KdStep step = kdStep( nd, qx, qy, qz, o );
      if ( step.farMin <= min( worst, cap ) && sp < uint32_t( kWideStack ) ) {
        if ( lane == 0 ) {
          st[4u * sp]      = step.farC;
          st[4u * sp + 1u] = uint32_t( step.far.o0 );
          st[4u * sp + 2u] = uint32_t( step.far.o1 );
          st[4u * sp + 3u] = uint32_t( step.far.o2 );
        }
        ++sp;
      }
      node = step.nearC;
      nd   = nodes[node];
    }
    if ( nd.dim < 0 ) {
      const uint32_t a = uint32_t( nd.a ), b = min( uint32_t( nd.b ), nTree );
      for ( uint32_t base = a; base < b; base += 64u ) {
        const uint32_t p    = base + lane;
        const uint32_t dist = p < b ? wideDist( qx, qy, qz, ptsTree[p] ) : kWideInf;
        unsigned long long take = __ballot( p < b && dist < worst && dist <= cap );
        while ( take ) {  // (at most 64 candidates, in tree order; the worst only falls)
          const int c = __ffsll( take ) - 1;
          take &= take - 1ull;
          const uint32_t d = uint32_t( __shfl( int( dist ), c ) );
          if ( d < worst ) {
            wideInsert( ld, li, K, count, d, base + uint32_t( c ), lane );
            if ( count == K ) worst = ld[K - 1u];
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    bool found = false;
    while ( sp > 0 ) {
      --sp;
      const uint32_t en = st[4u * sp], e0 = st[4u * sp + 1u], e1 = st[4u * sp + 2u], e2 = st[4u * sp + 3u];
      if ( e0 * e0 + e1 * e1 + e2 * e2 <= min( worst, cap ) ) {
        node = en, o = KdOffsets{int( e0 ), int( e1 ), int( e2 )};
        found = true;
        break;
      }
    }
    if ( !found || ++visits > nodeBudget ) break;
  }
  __builtin_amdgcn_wave_barrier();
  // (the list is full: K <= nTree, and everything within cap was visited; its positions are valid either way)
  if ( TRANSPOSED ) {
    for ( uint32_t e = lane; e < K; e += 64u ) out[size_t( e ) * outStride + j] = li[e];
  } else {
    uint32_t* row = out + size_t( queries ? j : perm[j] ) * K;
    for ( uint32_t e = lane; e < K; e += 64u ) row[e] = perm[min( li[e], nTree - 1u )];
  }
}

}  // namespace

int launchKnnWide( tmc2_ctx* ctx, const TreeDev& t, const Pt* d_queries, uint64_t nq, int k, uint32_t* d_out, bool transposed,
                   uint32_t outStride ) {
  if ( k > kWideMaxK ) {
    setError( "kdtree_search_wide: k=%d above %d (the result list of a wave lives in LDS)", k, kWideMaxK );
    return TMC2_E_UNSUPPORTED;
  }
  if ( k < 1 || uint64_t( k ) > t.n ) {
    setError( "kdtree_search_wide: k=%d larger than the cloud (%llu points), or below 1", k, (unsigned long long)t.n );
    return TMC2_E_INVALID;
  }
  if ( t.depth > kWideStack ) {
    setError( "kdtree_search_wide: k-d tree depth %d exceeds the traversal stack (%d)", t.depth, kWideStack );
    return TMC2_E_UNSUPPORTED;
  }
  if ( nq == 0 || nq > 0x7FFFFFF0ull || t.n > 0x7FFFFFF0ull ) {
    setError( "kdtree_search_wide: invalid argument" );
    return TMC2_E_INVALID;
  }
  const KdBox rb = kdBoxOf( t.lo, t.hi );
  for ( int d = 0; d < 3; ++d ) {
    if ( t.lo[d] < kWideMinCoord ) {
      setError( "kdtree_search_wide: coordinate %d below %d unsupported (squared distances are 32-bit)", t.lo[d], kWideMinCoord );
      return TMC2_E_UNSUPPORTED;
    }
  }
  StageScope     span( ctx, "knn_wide" );
  const uint32_t blocks = chunkedGrid( uint32_t( ( nq + kWideWaves - 1 ) / kWideWaves ) );
  const size_t   lds    = size_t( kWideWaves ) * ( 2u * size_t( k ) + 4u * kWideStack ) * sizeof( uint32_t );
  const uint32_t budget = uint32_t( std::min<uint64_t>( 4 * t.n + 64, 0xFFFFFFF0ull ) );  // (a tree of n points has fewer than 2 n nodes)
  if ( transposed )
    hipLaunchKernelGGL( knnWideKernel<true>, dim3( blocks ), dim3( 64 * kWideWaves ), lds, ctx->stream, t.ptsTree, t.perm, t.nodes, rb, d_queries,
                        uint32_t( nq ), uint32_t( t.n ), uint32_t( k ), budget, d_out, outStride );
  else
    hipLaunchKernelGGL( knnWideKernel<false>, dim3( blocks ), dim3( 64 * kWideWaves ), lds, ctx->stream, t.ptsTree, t.perm, t.nodes, rb, d_queries,
                        uint32_t( nq ), uint32_t( t.n ), uint32_t( k ), budget, d_out, outStride );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

}  // namespace tmc2

using namespace tmc2;

extern "C" int tmc2_kdtree_search_wide( tmc2_frame* f, const int16_t* queries, uint64_t nq, int k, uint32_t* idx ) {
  if ( !f || !idx || f->n == 0 || ( queries ? nq == 0 || nq > 0x7FFFFFF0ull : nq != f->n ) ) {
    setError( "kdtree_search_wide: invalid argument (without queries, nq is the frame's point count)" );
    return TMC2_E_INVALID;
  }
  if ( k > kWideMaxK ) {  // (checked before anything is sized by k)
    setError( "kdtree_search_wide: k=%d above %d (the result list of a wave lives in LDS)", k, kWideMaxK );
    return TMC2_E_UNSUPPORTED;
  }
  if ( k < 1 || uint64_t( k ) > f->n ) {
    setError( "kdtree_search_wide: k=%d larger than the cloud (%llu points), or below 1", k, (unsigned long long)f->n );
    return TMC2_E_INVALID;
  }
  ApiScope scope( f->ctx );
  TMC2_TRY( f->ensureTree() );
  hipStream_t      s = f->ctx->stream;
  DevBuf<Pt>       d_q;
  DevBuf<uint32_t> d_idx;
  std::vector<Pt>  q;
  if ( queries ) {
    q.resize( nq );
    for ( uint64_t i = 0; i < nq; ++i ) {
      q[i] = Pt{queries[3 * i], queries[3 * i + 1], queries[3 * i + 2], 0};
      for ( int d = 0; d < 3; ++d )
        if ( queries[3 * i + d] < kWideMinCoord ) {
          setError( "kdtree_search_wide: coordinate %d below %d unsupported (squared distances are 32-bit)", int( queries[3 * i + d] ), kWideMinCoord );
          return TMC2_E_UNSUPPORTED;
        }
    }
    TMC2_TRY( d_q.alloc( nq ) );
    TMC2_HIP( hipMemcpyAsync( d_q.p, q.data(), nq * sizeof( Pt ), hipMemcpyHostToDevice, s ) );
  }
  TMC2_TRY( d_idx.alloc( nq * size_t( k ) ) );
  TMC2_TRY( launchKnnWide( f->ctx, f->tree.view( QueryBox::Any ), queries ? d_q.p : nullptr, nq, k, d_idx.p, false, 0 ) );
  TMC2_HIP( hipMemcpyAsync( idx, d_idx.p, nq * size_t( k ) * 4, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  return TMC2_OK;
}
