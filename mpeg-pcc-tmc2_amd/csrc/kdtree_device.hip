// kdtree_device.hip -- construction of the nanoflann-identical k-d tree ON the device (S1).
//
// Replaces PCCKdTree::init (reference: source/lib/PccLibCommon/source/PCCKdTree.cpp:56-59), i.e. nanoflann's
// buildIndex / divideTree / middleSplit_ / planeSplit (dependencies/nanoflann/nanoflann.hpp:858-866, 1041-1181)
// for int16 3-D points and leaf size 10.  kdtree_build.cpp is the same algorithm on the host (kept for the host-only
// entry point and as the cross-check of this one); see its header for why the tree has to be IDENTICAL, permutation
// included.
//
// The reference builds depth-first and partitions each node with a sequential two-pass Hoare sweep.  Here the tree is
// built LEVEL by level, all nodes of a level at once, with every per-node step turned into a data-parallel pass over
// the points (tree-order arrays, segment id per point):
//   * ranges  : segmented wave reduction + atomicMin/Max per node (one pass gives the ranges of all three dimensions);
//   * split   : per node -- widest loose-box dimension / largest spread, midpoint clamped to the range (as the host);
//   * partition: what the Hoare sweep leaves behind is closed-form.  With L = "value < cut", nL = #L: the sweep ends with
//     every L in [0,nL) and swaps, in order, the i-th misplaced non-L from the left with the i-th misplaced L from the
//     right; elements already on their side never move.  A prefix sum of the class flag gives every misplaced element
//     its rank, the right-hand ones publish their position by rank, the left-hand ones swap with it.  The second sweep
//     ("value <= cut" on [nL, count)) is the same on the sub-range.  lim1 / lim2 fall out of the same prefix sums;
//   * children: node ids and next-level slots from atomic counters (ids are arbitrary: the traversal follows explicit
//     child ids; only the ROOT must be node 0), loose boxes handed down, and each child reports its tight range to
//     the parent's divlow / divhigh when it is measured at the next level.
// A level is five short launches over <= n points (round 5: class flags + prefix sum, first swaps through partner lists, second
// flags, second swaps + landing, decide -- see "round 5's level passes" below); how many levels the passes run is read back once
// per tree (the count of the previous tree of this size is queued speculatively).
// The level passes only carry the top of the tree: a segment of at most 16 384 points (option KD_HUGEMAX) leaves them for ONE
// workgroup that cuts it into pieces in global memory (hugeSegmentsKernel), and a piece of at most kPieceMax = 4 096 points is
// finished by one workgroup with its points in LDS, ALL nodes of a depth at once (pieceKernel).
// Rounds 2-4 finished the subtrees with three other tiers (a workgroup per <= 8 192-point segment with a wavefront per node, a
// wavefront per <= 512-point subtree, single lanes below 32 points) and round 4 ran its own five launches per level; round 5
// kept both behind options (KD_FORM=tiers, KD_LEVELS=r4) as a third cross-check next to the host builder and the oracle; round 6
// took them out of the library (~ 950 lines: git show 5d8d688:mpeg-pcc-tmc2_amd/csrc/kdtree_device.hip).
// (A single persistent launch with grid-wide barriers was measured too: on this multi-XCD part every barrier is an L2
// write-back + invalidate per workgroup, ~45 us per pass, and the builds of concurrent frames serialise.  Separate
// launches leave the gaps of one frame to the passes of the others.)
#include <algorithm>
#include <cstring>

#include "internal.h"
#include "loads.h"
#include "wave.h"

namespace tmc2 {
namespace {

constexpr uint32_t kNone      = 0xFFFFFFFFu;
constexpr int      kBlock     = 256;
constexpr int      kWaves     = kBlock / 64;
constexpr int      kScanTile  = kBlock * 8;
constexpr int      kLeafMax   = 10;
constexpr int      kMaxLevels = 64;    // = the traversal stack of the k-NN kernels

struct BuildSeg {
  uint32_t begin, end;    // range in tree order
  uint32_t node, parent;  // own node id; parent's node id (kNone for the root)
  int32_t  mn[3], mx[3];  // tight range of the points (atomics)
  int16_t  lo[3], hi[3];  // loose box handed down by the parent (root: unused, its box is its range)
  uint8_t  side, pdim;    // which child of the parent we are, and the parent's cut dimension
  uint8_t  split, cutDim;
  int32_t  cut;
  uint32_t mid;           // begin + idx: first point of the right child
  uint32_t slot;          // next-level slot of the left child (right = slot + 1)
};

// a segment handed to finishSubtreesKernel: its slice of the tree-order arrays, its (allocated) node id, loose box, level
struct RetiredSeg {
  uint32_t begin, end, node, level;
  int16_t  lo[3], hi[3];
  int32_t  root;  // 1: the root of the whole tree (its loose box is its tight range)
};

// a segment handed to hugeSegmentsKernel: the same, with the tight ranges the level pass measured
struct HugeSeg {
  uint32_t begin, end, node, level;
  int16_t  lo[3], hi[3];
  int32_t  root;
  int32_t  mn[3], mx[3];
};

struct BuildArgs {
  const Pt* pts;
  uint32_t  n, tiles;
  Pt*       P;
  uint32_t *perm, *seg;
  BuildSeg *segA, *segB;
  KdNode*   nodes;
  uint32_t *loc1, *loc2, *tile1, *tile2;  // tile1 / tile2: [tiles + 1] tile totals, scanned in place (+ total)
  uint32_t* counts;     // [kMaxLevels + 1] segments per level
  uint32_t* nodeCount;
  int32_t*  rootBox;    // [6]
  uint32_t* levels;     // out: number of levels
  RetiredSeg* retired;  // the pieces: disjoint segments of more than kLeafMax and at most kPieceMax points
  uint32_t*   retiredCount;
  uint32_t*   bigCount;
  HugeSeg*    huge;     // segments of more than kPieceMax and at most hugeMax points (hugeSegmentsKernel)
  uint32_t*   hugeCount;
  uint32_t    hugeMax;  // (>= splitMax; == splitMax: no such segments)
  uint32_t    retireMax, splitMax;  // both kPieceMax (round 4's tiers had two thresholds)
  struct LvSeg *lvA, *lvB;          // round 5's level passes: the segments of a level (by level parity)
  uint16_t*   list;                 // [n rounded up to whole tiles] positions not of a sweep's class, compacted per tile
  struct LvPartial* partial;        // [n / (kLandBlock * kLandRounds) + 1] what a workgroup of the landing pass found for the two children of its segment
  unsigned long long* pieceProfile;  // option KD_PIECE_PROFILE: wall-clock ticks (10 ns) thread 0 of every workgroup spent between the barriers of a depth
  uint32_t    decideRng;            // segments of a level whose ranges the decide pass folds in LDS (kDecideRng; 0: option KD_DECIDE=global, the path of larger levels)
  uint32_t*   finishDepth;  // out: levels reached inside the retired subtrees
  uint32_t*   ticket;       // workgroups of pieceKernel that are done (the last one publishes finishDepth to the host)
  // page-locked words of the context (tmc2_ctx::answerLine) the host reads after its synchronisation instead of copying:
  volatile uint32_t* hostSmall;  // lvDecideKernel: the whole counter block (kMaxLevels + 16 words); null: this launch does not publish
  volatile uint32_t* hostDepth;  // pieceKernel's last workgroup: finishDepth
};

struct SplitRule {
  int     dim;
  int32_t cut;
};
// nanoflann's middleSplit_ on a loose box and the tight ranges of the points (as splitRule() above / kdtree_build.cpp)
__device__ __forceinline__ SplitRule splitOf( const int16_t ( &lo )[3], const int16_t ( &hi )[3], const int32_t ( &mn )[3],
                                              const int32_t ( &mx )[3] ) {
  const int32_t maxSpan = max( int32_t( hi[0] ) - lo[0], max( int32_t( hi[1] ) - lo[1], int32_t( hi[2] ) - lo[2] ) );
  SplitRule     r;
  r.dim              = 0;
  int32_t bestSpread = -1;
#pragma unroll
  for ( int d = 0; d < 3; ++d ) {
    if ( double( int32_t( hi[d] ) - lo[d] ) > ( 1.0 - 0.00001 ) * double( maxSpan ) ) {
      const int32_t spread = mx[d] - mn[d];
      if ( spread > bestSpread ) {
        bestSpread = spread;
        r.dim      = d;
      }
    }
  }
  const int32_t l = r.dim == 0 ? lo[0] : ( r.dim == 1 ? lo[1] : lo[2] ), h = r.dim == 0 ? hi[0] : ( r.dim == 1 ? hi[1] : hi[2] );
  const int32_t a = r.dim == 0 ? mn[0] : ( r.dim == 1 ? mn[1] : mn[2] ), b = r.dim == 0 ? mx[0] : ( r.dim == 1 ? mx[1] : mx[2] );
  r.cut           = min( max( ( l + h ) / 2, a ), b );
  return r;
}

// ---- segments of kSplitMax .. hugeMax points: one workgroup each, points where they are (global memory, L2-resident), the
// WHOLE workgroup on one node after the other, depth by depth, until the pieces fit splitSegmentsKernel.
// Why: a level pass is five launches over ALL n points, and from the level on where the segments are a few tens of thousands of
// points the chip streams the arrays five times per level to move a few elements inside each segment.  Sixteen frames in
// flight pay for chip time, not for latency: ~ 20 workgroups busy for the time of those levels leave the rest of the chip to
// the other frames.  Same closed-form sweeps as everywhere (the i-th misplaced element from the left swaps with the i-th from
// the right), in three passes over a node instead of nine:
//   * one pass lists the positions of the ">= c" elements and of the "< c" elements (both ascending, in the node's slices of
//     loc1 / loc2, which the level passes no longer use) -- the number of "< c" elements IS the sweep's edge nL, the misplaced
//     elements on the left are the head of the first list (positions < nL), their partners the tail of the second, read
//     backwards;
//   * the same on [nL, count) with c + 1 for the second sweep;
//   * one pass gives the tight ranges of both children (divlow / divhigh are two of the twelve numbers), so the children start
//     with their ranges known.
// Four elements per thread and pass iteration (independent loads: the passes are bound by load latency, not by bandwidth).
constexpr int      kHugeWaves = 16;
constexpr uint32_t kHugeLimit = 131072;                                 // largest hugeMax
constexpr int      kHugeNodes = 2 * int( kHugeLimit / 4096 ) + 4;  // nodes of more than splitMax (>= 4096) points at one depth
struct HugeNode {
  uint32_t begin, end;  // range inside the segment
  uint32_t node;
  int16_t  lo[3], hi[3];  // loose box
  int16_t  mn[3], mx[3];  // tight ranges
  uint16_t depth;
};

// Lists the positions of pts[0..count) with coordinate >= c (listGE) and < c (listLT), both ascending; returns the number of
// ">= c" elements.  waveCnt: LDS [2][kHugeWaves].
__device__ __forceinline__ uint32_t blockClassLists( const Pt* pts, uint32_t count, int dim, int32_t c, uint32_t* listGE,
                                                     uint32_t* listLT, uint32_t* waveCnt ) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t  mGE = 0, mIn = 0;
  int       buf = 0;
  for ( uint32_t base = 0; base < count; base += 4u * blockDim.x, buf ^= 1 ) {
    const uint32_t i0 = base + 4u * threadIdx.x;
    bool           ge[4];
    uint32_t       cGE = 0, cIn = 0;
    Words2           pw[4];  // (the four loads ahead of one wait)
#pragma unroll
    for ( int j = 0; j < 4; ++j ) pw[j] = *reinterpret_cast<const Words2*>( pts + ( i0 + j < count ? i0 + j : 0u ) );
    pin( pw[0], pw[1], pw[2], pw[3] );
#pragma unroll
    for ( int j = 0; j < 4; ++j ) {
      const bool    in = i0 + j < count;
      const int32_t x  = ptCoord( pw[j], dim );
      ge[j]            = in && x >= c;
      cGE += uint32_t( ge[j] ), cIn += uint32_t( in );
    }
    const uint32_t inc = waveInclusive( cGE | ( cIn << 16 ), lane );  // (a wave holds at most 256 elements: both counts fit 16 bits)
    if ( lane == 63 ) waveCnt[buf * kHugeWaves + wave] = inc;
    __syncthreads();  // (the other buffer is written next: whoever still reads this one has passed this barrier by then)
    uint32_t before = 0, total = 0;
#pragma unroll
    for ( int w = 0; w < kHugeWaves; ++w ) {
      const uint32_t cw = waveCnt[buf * kHugeWaves + w];
      total += cw;
      before += w < wave ? cw : 0u;
    }
    before += inc - ( cGE | ( cIn << 16 ) );
    uint32_t atGE = mGE + ( before & 0xFFFFu ) + 0u, atIn = mIn + ( before >> 16 );
    // (before / total: sums of packed pairs; the low halves cannot carry -- at most 4 096 elements per iteration)
#pragma unroll
    for ( int j = 0; j < 4; ++j ) {
      if ( i0 + j < count ) {
        if ( ge[j] )
          listGE[atGE] = i0 + j;
        else
          listLT[atIn - atGE] = i0 + j;
        atGE += uint32_t( ge[j] ), ++atIn;
      }
    }
    mGE += total & 0xFFFFu, mIn += total >> 16;
  }
  return mGE;
}

// One sweep by the workgroup on pts[0..count): left class "value < c".  Returns nL, the number of elements of the left class.
__device__ __forceinline__ uint32_t blockSweep( Pt* pts, uint32_t* id, uint32_t count, int dim, int32_t c, uint32_t* listGE,
                                                uint32_t* listLT, uint32_t* waveCnt ) {
  const uint32_t nGE = blockClassLists( pts, count, dim, c, listGE, listLT, waveCnt ), nL = count - nGE;
  __syncthreads();
  for ( uint32_t t = threadIdx.x; t < min( nGE, nL ); t += blockDim.x ) {
    uint32_t x = listGE[t], y = listLT[nL - 1u - t];  // (both entries together: t < nL)
    pin( x, y );
    if ( x >= nL ) break;  // (ascending: nothing misplaced from here on)
    const Pt       px = pts[x], py = pts[y];
    const uint32_t ix = id[x], iy = id[y];
    pts[x] = py, pts[y] = px, id[x] = iy, id[y] = ix;
  }
  __syncthreads();
  return nL;
}

__global__ __launch_bounds__( 64 * kHugeWaves ) void hugeSegmentsKernel( BuildArgs a ) {
  __shared__ HugeNode sNode[2][kHugeNodes];
  __shared__ uint32_t sCount[2], waveCnt[2 * kHugeWaves];
  __shared__ int32_t  red[kHugeWaves][12];
  const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t total = *a.hugeCount;
  for ( uint32_t s = blockIdx.x; s < total; s += gridDim.x ) {
    const HugeSeg seg = a.huge[s];
    __syncthreads();  // (a slower wavefront may still be reading the previous segment's last sCount)
    if ( threadIdx.x == 0 ) {
      HugeNode r;
      r.begin = 0, r.end = seg.end - seg.begin, r.node = seg.node, r.depth = 0;
      for ( int d = 0; d < 3; ++d ) r.lo[d] = seg.lo[d], r.hi[d] = seg.hi[d], r.mn[d] = int16_t( seg.mn[d] ), r.mx[d] = int16_t( seg.mx[d] );
      sNode[0][0] = r;
      sCount[0] = 1, sCount[1] = 0;
    }
    __syncthreads();
    int cur = 0;
    for ( uint32_t depth = 0;; ++depth ) {
      const uint32_t nCur = sCount[cur];
      if ( nCur == 0 ) break;
      for ( uint32_t t = 0; t < nCur; ++t ) {  // (uniform over the workgroup)
        const HugeNode q     = sNode[cur][t];
        const uint32_t count = q.end - q.begin;
        if ( uint32_t( q.depth ) + seg.level >= uint32_t( kMaxLevels ) - 2u ) {  // deeper than the k-NN traversal stack: refused
          if ( threadIdx.x == 0 ) atomicMax( a.finishDepth, 0x10000u );
          continue;
        }
        Pt*       pts = a.P + seg.begin + q.begin;
        uint32_t* id  = a.perm + seg.begin + q.begin;
        int32_t   mn[3], mx[3];
        const bool isRoot = seg.root != 0 && depth == 0;  // the tree's root: its loose box is its tight range
        int16_t    lo[3], hi[3];
        for ( int d = 0; d < 3; ++d ) mn[d] = q.mn[d], mx[d] = q.mx[d], lo[d] = isRoot ? q.mn[d] : q.lo[d], hi[d] = isRoot ? q.mx[d] : q.hi[d];
        const SplitRule rule  = splitOf( lo, hi, mn, mx );
        uint32_t*       listA = a.loc1 + seg.begin + q.begin;
        uint32_t*       listB = a.loc2 + seg.begin + q.begin;
        const uint32_t  lt    = blockSweep( pts, id, count, rule.dim, rule.cut, listA, listB, waveCnt );
        const uint32_t  le    = lt + blockSweep( pts + lt, id + lt, count - lt, rule.dim, rule.cut + 1, listA, listB, waveCnt );
        const uint32_t  half  = count / 2;
        const uint32_t  idx   = lt > half ? lt : ( le < half ? le : half );
        // tight ranges of the two children
        int32_t r[12];
#pragma unroll
        for ( int k = 0; k < 12; ++k ) r[k] = ( k % 6 ) < 3 ? 0x7FFFFFFF : int32_t( 0x80000000 );
        for ( uint32_t base = 0; base < count; base += 4u * blockDim.x ) {
          Pt p[4];
#pragma unroll
          for ( int j = 0; j < 4; ++j ) {
            const uint32_t i = base + j * blockDim.x + threadIdx.x;
            p[j]             = pts[i < count ? i : 0u];
          }
#pragma unroll
          for ( int j = 0; j < 4; ++j ) {
            const uint32_t i = base + j * blockDim.x + threadIdx.x;
            if ( i < count ) {
              const int o = i < idx ? 0 : 6;
              if ( o == 0 ) {
                r[0] = min( r[0], int32_t( p[j].x ) ), r[1] = min( r[1], int32_t( p[j].y ) ), r[2] = min( r[2], int32_t( p[j].z ) );
                r[3] = max( r[3], int32_t( p[j].x ) ), r[4] = max( r[4], int32_t( p[j].y ) ), r[5] = max( r[5], int32_t( p[j].z ) );
              } else {
                r[6] = min( r[6], int32_t( p[j].x ) ), r[7] = min( r[7], int32_t( p[j].y ) ), r[8] = min( r[8], int32_t( p[j].z ) );
                r[9] = max( r[9], int32_t( p[j].x ) ), r[10] = max( r[10], int32_t( p[j].y ) ), r[11] = max( r[11], int32_t( p[j].z ) );
              }
            }
          }
        }
#pragma unroll
        for ( int off = 32; off > 0; off >>= 1 )
#pragma unroll
          for ( int k = 0; k < 12; ++k ) {
            const int32_t o = __shfl_xor( r[k], off, 64 );
            r[k]            = ( k % 6 ) < 3 ? min( r[k], o ) : max( r[k], o );
          }
        if ( lane == 0 )
          for ( int k = 0; k < 12; ++k ) red[wave][k] = r[k];
        __syncthreads();
        // the wavefronts' partial ranges, one of the twelve numbers per thread.  (Thread 0 folding all 16 x 12 was unrolled
        // into 192 LDS reads in flight at once: the kernel sat at its 128-VGPR cap with 596 bytes of private memory per lane
        // and spilled inside the sweeps' loops; now 101 VGPRs and none.)
        if ( threadIdx.x < 12 ) {
          int32_t v = red[0][threadIdx.x];
          for ( int w = 1; w < kHugeWaves; ++w ) v = ( threadIdx.x % 6 ) < 3 ? min( v, red[w][threadIdx.x] ) : max( v, red[w][threadIdx.x] );
          red[0][threadIdx.x] = v;
        }
        __syncthreads();
        if ( threadIdx.x == 0 ) {
#pragma unroll
          for ( int k = 0; k < 12; ++k ) r[k] = red[0][k];
          const uint32_t id0 = atomicAdd( a.nodeCount, 2u );
          KdNode         nd;
          nd.a = int32_t( id0 ), nd.b = int32_t( id0 + 1 ), nd.divlow = int16_t( r[3 + rule.dim] ), nd.divhigh = int16_t( r[6 + rule.dim] ),
          nd.dim = rule.dim;
          a.nodes[q.node] = nd;
          HugeNode child[2];
          child[0].begin = q.begin, child[0].end = q.begin + idx, child[0].node = id0;
          child[1].begin = q.begin + idx, child[1].end = q.end, child[1].node = id0 + 1;
          for ( int c = 0; c < 2; ++c ) {
            child[c].depth = uint16_t( q.depth + 1 );
            for ( int d = 0; d < 3; ++d )
              child[c].lo[d] = lo[d], child[c].hi[d] = hi[d], child[c].mn[d] = int16_t( r[6 * c + d] ), child[c].mx[d] = int16_t( r[6 * c + 3 + d] );
          }
          const int16_t cut = int16_t( rule.cut );
          if ( rule.dim == 0 ) child[0].hi[0] = cut, child[1].lo[0] = cut;
          if ( rule.dim == 1 ) child[0].hi[1] = cut, child[1].lo[1] = cut;
          if ( rule.dim == 2 ) child[0].hi[2] = cut, child[1].lo[2] = cut;
          for ( int c = 0; c < 2; ++c ) {
            const uint32_t cc = child[c].end - child[c].begin, level = seg.level + child[c].depth;
            if ( cc <= uint32_t( kLeafMax ) ) {
              KdNode leaf;
              leaf.a = int32_t( seg.begin + child[c].begin ), leaf.b = int32_t( seg.begin + child[c].end ), leaf.divlow = leaf.divhigh = 0,
              leaf.dim = -1;
              a.nodes[child[c].node] = leaf;
              atomicMax( a.finishDepth, level + 1u );
            } else if ( cc <= a.retireMax ) {  // to the piece kernel
              RetiredSeg rs;
              rs.begin = seg.begin + child[c].begin, rs.end = seg.begin + child[c].end, rs.node = child[c].node, rs.level = level, rs.root = 0;
              for ( int d = 0; d < 3; ++d ) rs.lo[d] = child[c].lo[d], rs.hi[d] = child[c].hi[d];
              a.retired[atomicAdd( a.retiredCount, 1u )] = rs;
            } else {
              sNode[cur ^ 1][sCount[cur ^ 1]++] = child[c];
            }
          }
        }
        __syncthreads();
      }
      if ( threadIdx.x == 0 ) sCount[cur] = 0;
      cur ^= 1;
      __syncthreads();
    }
  }
}

// ---- pieces of at most kPieceMax points: ONE workgroup each, points in LDS, ALL nodes of a depth at once (round 5) --------
// The same level-parallel closed form as the chip-wide passes above, with workgroup barriers where those have kernel boundaries
// and LDS where those have global memory: per depth, every record (= node of more than kLeafMax points) of the piece is
// split at the same time -- class flags and ONE workgroup prefix sum per sweep, the misplaced right-hand elements publish
// their position by rank (from the right) in the node's own slice of a list, the misplaced left-hand elements swap with the
// entry of their rank (from the left); the children's tight ranges (and with them the parent's divlow / divhigh) come from one
// segmented wavefront reduction keyed by (record, side) once the elements have landed.  A thread owns K consecutive
// positions and keeps what it has read of them (record, its range and rule, the prefix sums) in registers from pass to pass.
// Replaces hugeSegmentsKernel / splitSegmentsKernel / finishSubtreesKernel (a wavefront per node, depth by depth, single lanes
// running nanoflann's recursion below 32 points: 0.3 + 0.2 + 0.25 ms per tree, most of it divergence and one wavefront on a
// node of thousands of points); here nothing diverges and nothing is sequential but the depths themselves.
// The barriers between the passes order LDS only (s_waitcnt lgkmcnt(0) + s_barrier): the node records a pass writes to global
// memory and the one returning atomic per depth (node ids of the NEXT depth's children, asked for a few passes ahead) stay
// in flight across them -- nobody in the workgroup reads those back.
constexpr int      kPieceMax  = 4096;
constexpr int      kPieceRecs = kPieceMax / ( kLeafMax + 1 ) + 2;  // records of one depth: disjoint, more than kLeafMax points each
constexpr uint16_t kNoRec     = 0xFFFFu;
constexpr uint32_t kNoKey     = 0xFFFFFFFFu;

struct alignas( 8 ) PieceRec {
  uint16_t begin, end;     // [0] what the flag passes read: range inside the piece, the split rule
  int16_t  cut;
  uint8_t  dim, unused0;
  uint16_t edge1, rb1;     // [8] first sweep: end of the "< cut" class, prefix at begin
  uint16_t edge2, rb2;     //     second sweep: end of the "<= cut" class, prefix at edge1
  uint16_t mid;            // [16] first position of the right child
  uint16_t child[2];       //      records of the children at the next depth (kNoRec: a leaf)
  uint16_t unused1;
  uint32_t node;           // own node id
  int32_t  lmax, rmin;     // tight bounds of the two children on the cut dimension (divlow / divhigh)
  int16_t  lo[3], hi[3];   // loose box
  int32_t  mn[3], mx[3];   // tight range (LDS atomics)
};
static_assert( sizeof( PieceRec ) == 72, "PieceRec layout" );
struct PieceHot0 {
  uint32_t be, dc;  // begin | end << 16 ;  cut (16 bits) | dim << 16
};
struct PieceHot1 {
  uint32_t e1rb1, e2rb2;
};
struct PieceHot2 {
  uint32_t midc0, c1;
};

__device__ __forceinline__ void pieceBarrier() { asm volatile( "s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory" ); }

typedef short pkShort2 __attribute__( ( ext_vector_type( 2 ) ) );
__device__ __forceinline__ uint32_t pkMin( uint32_t a, uint32_t b ) {
  return __builtin_bit_cast( uint32_t, __builtin_elementwise_min( __builtin_bit_cast( pkShort2, a ), __builtin_bit_cast( pkShort2, b ) ) );
}
__device__ __forceinline__ uint32_t pkMax( uint32_t a, uint32_t b ) {
  return __builtin_bit_cast( uint32_t, __builtin_elementwise_max( __builtin_bit_cast( pkShort2, a ), __builtin_bit_cast( pkShort2, b ) ) );
}
__device__ __forceinline__ uint32_t pk2( int lo16, int hi16 ) { return ( uint32_t( lo16 ) & 0xFFFFu ) | ( uint32_t( hi16 ) << 16 ); }
__device__ __forceinline__ int      pkLo( uint32_t v ) { return int( int16_t( v & 0xFFFFu ) ); }
__device__ __forceinline__ int      pkHi( uint32_t v ) { return int( int16_t( v >> 16 ) ); }

// exclusive prefix sum over the workgroup of one value per thread; waveTot: LDS [WAVES] -- the caller alternates between two
// of them, so that the next scan may start while slow wavefronts still read this one's
template <int WAVES>
__device__ __forceinline__ uint32_t pieceScan( uint32_t v, uint32_t* waveTot ) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = waveInclusive( v, lane );
  if ( lane == 63 ) waveTot[wave] = inc;
  pieceBarrier();
  uint32_t before = 0;
#pragma unroll
  for ( int w = 0; w < WAVES; w += 4 ) {
    const uint4 t = *reinterpret_cast<const uint4*>( waveTot + w );
    before += ( w + 0 < wave ? t.x : 0u ) + ( w + 1 < wave ? t.y : 0u ) + ( w + 2 < wave ? t.z : 0u ) + ( w + 3 < wave ? t.w : 0u );
  }
  return before + inc - v;
}

// Segmented min / max over a wavefront of (x, y, z) packed as A = (x, y) under min, B = (x, y) under max, C = (z, ~z) under min:
// lanes with equal keys are contiguous; afterwards the first lane of every run holds the run's values.  Returns: this lane is
// such a first lane (of a real key).
__device__ __forceinline__ bool waveSegMinMaxPacked( uint32_t key, uint32_t& A, uint32_t& B, uint32_t& C, int lane ) {
#pragma unroll
  for ( int off = 1; off < 64; off <<= 1 ) {
    const uint32_t ok = __shfl_down( key, off, 64 );
    const uint32_t oa = __shfl_down( A, off, 64 ), ob = __shfl_down( B, off, 64 ), oc = __shfl_down( C, off, 64 );
    if ( lane + off < 64 && ok == key ) A = pkMin( A, oa ), B = pkMax( B, ob ), C = pkMin( C, oc );
  }
  const uint32_t pk = __shfl_up( key, 1, 64 );
  return key != kNoKey && ( lane == 0 || pk != key );
}

__device__ __forceinline__ void ldsMin( int32_t* slot, int32_t v ) {
  if ( v < *reinterpret_cast<volatile int32_t*>( slot ) ) atomicMin( slot, v );
}
__device__ __forceinline__ void ldsMax( int32_t* slot, int32_t v ) {
  if ( v > *reinterpret_cast<volatile int32_t*>( slot ) ) atomicMax( slot, v );
}


// ---- round 5's level passes -----------------------------------------------------------------------------------------------
// The same five steps per level (ranges; flags + prefix sum; first swaps; second flags + prefix sum; second swaps + children),
// re-cut so that every launch is a SHORT chain of dependent loads -- a level pass over 0.84 M points moves a few megabytes, what it
// costs is the number of L2 round trips one thread makes in a row:
//   * a misplaced element finds its partner through a LIST instead of a binary search over the prefix sums (20 dependent loads
//     near the root): the flag passes compact the tile-local offsets of the elements that are NOT of the class per tile; the
//     partner of left-rank r is the element of global rank U(end) - 1 - r among those, its tile found by a search of the tile
//     totals in LDS, its offset by one load;
//   * the split rule, the children's slots and node ids are decided once per segment by one small launch (lvDecideKernel:
//     prefix sum over the segments that split) instead of being re-derived per point with fp64 / handed out by atomics;
//   * the children's tight ranges are gathered by the pass that lands the elements (a segmented wavefront reduction keyed by the
//     child; what a swap moves reports on its own), so the separate range pass and its re-labelling of every point are gone;
//   * the first sweep's edge is stored by the thread that sits on the segment's first position, the children are written by
//     that thread of the last pass.
// Launches per level: flags, swaps, flags, swaps + landing, decide (tiny).  Swap for swap nanoflann's planeSplit
// (nanoflann.hpp:1154-1181), as everything in this file.
// The chains as the code object has them (what a thread waits for in a row; loads of one step are issued together, ahead of
// the branches that use them, at clamped addresses where a position is retired or lies beyond n -- loads.h):
//   * lvFlagKernel, per tile, a thread on its 8 consecutive positions: the 8 seg words (two 16-byte loads) -> the cut word of
//     the 8 records (second sweep: cut word and edge1, one 8-byte load each) together with the 8 points (four 16-byte loads).
//     loc goes out as two 16-byte stores.  The second sweep's reset of the children's ranges: cutInfo and slot together,
//     then a 16- and an 8-byte store per child.  (Was: seg, record, point one after the other for each of the 8 positions.)
//   * lvSwapTwoKernel, per position: seg -> { record rows 0, 1, 2, P[i], loc2[i], perm[i] } -> { loc2[edge1], loc2[end] } ->
//     list -> { P[j], perm[j] }; the thread on a segment's first position builds both children in registers from the rows it
//     holds and stores rows 0 .. 2 of each whole; lvReport reads its six words ahead of one wait and then issues the
//     atomics it still needs with no wait between them.
//   * lvSwapOneKernel and lvDecideKernel read their records field by field as before: the batched forms (SwapOne: 5 trips
//     instead of 8, also with a thread's two positions sharing every trip; Decide: the record's rows and the six range words
//     in two batches) measured no faster, alone or with 16 frames in flight -- the first swap pass is bound by its scattered
//     swaps, not by its chain.  Fetching P[i] / loc[i] / perm[i] before seg[i] is known (a trip less, but for retired positions
//     too) measured no better either.  profiles/kdtree_level_loads.txt has the figures.
// The record is read and written in ROWS of 16 bytes (lvRow / lvStoreRow): row 0 is what every position of a sweep needs, row 1
// what the landing pass adds, row 2 the box a segment's first position hands down; the tight range (atomics) follows and is
// only ever touched word by word.  80 bytes, 16-byte aligned: a row is one global_load_dwordx4.
struct alignas( 16 ) LvSeg {
  uint32_t begin, end;     // [ 0] range in tree order
  uint32_t cutInfo;        //      cut (16 bits) | cutDim << 16 | splits << 24
  uint32_t edge1;          //      first position not of the first sweep's left class (stored by the first swap pass)
  uint32_t slot;           // [16] the children's segments at the next level: slot, slot + 1
  uint32_t childNode;      //      ... and their node ids: childNode, childNode + 1
  uint32_t node, parent;   //      own node id; parent's node id (kNone for the root)
  int16_t  lo[3], hi[3];   // [32] loose box handed down by the parent (root: unused, its box is its range)
  uint8_t  side, pdim;     //      which child of the parent we are, and the parent's cut dimension
  uint16_t unused;
  int32_t  mn[3], mx[3];   // [48] tight range of the points (atomics)
  uint32_t pad[2];
};
static_assert( sizeof( LvSeg ) == 80 && offsetof( LvSeg, slot ) == 16 && offsetof( LvSeg, lo ) == 32 && offsetof( LvSeg, mn ) == 48, "LvSeg rows" );

__device__ __forceinline__ Words4 lvRow( const LvSeg* q, int row ) { return reinterpret_cast<const Words4*>( q )[row]; }
__device__ __forceinline__ void lvStoreRow( LvSeg* q, int row, Words4 w ) { reinterpret_cast<Words4*>( q )[row] = w; }

constexpr int kLandBlock = 256;  // the landing pass: one record of the children's ranges per workgroup (measured: 1 024-thread workgroups quarter the records the decide pass folds -- 14 -> 7 us -- and cost the landing pass itself 18 -> 32 us)
constexpr int kLandRounds = 2;  // ... of consecutive rounds of kLandBlock positions: their records are merged where they name the same segment
struct LvPartial {
  uint32_t slot;  // left child's segment at the next level (kNone: this workgroup reported on its own / had nothing)
  uint32_t v[6];  // packed (mn x|y, mx x|y, mn z | ~mx z) of the left and of the right child
  uint32_t unused;
};

__device__ __forceinline__ void lvReport( LvSeg* child, int mnx, int mny, int mnz, int mxx, int mxy, int mxz ) {
  // the six (possibly stale) words ahead of one wait, then the atomics that are still needed, none of them waited for
  uint32_t s0 = uint32_t( loadStaleOk( &child->mn[0] ) ), s1 = uint32_t( loadStaleOk( &child->mn[1] ) ), s2 = uint32_t( loadStaleOk( &child->mn[2] ) );
  uint32_t s3 = uint32_t( loadStaleOk( &child->mx[0] ) ), s4 = uint32_t( loadStaleOk( &child->mx[1] ) ), s5 = uint32_t( loadStaleOk( &child->mx[2] ) );
  pin( s0, s1, s2, s3, s4, s5 );
  if ( mnx < int32_t( s0 ) ) atomicMin( &child->mn[0], mnx );
  if ( mny < int32_t( s1 ) ) atomicMin( &child->mn[1], mny );
  if ( mnz < int32_t( s2 ) ) atomicMin( &child->mn[2], mnz );
  if ( mxx > int32_t( s3 ) ) atomicMax( &child->mx[0], mxx );
  if ( mxy > int32_t( s4 ) ) atomicMax( &child->mx[1], mxy );
  if ( mxz > int32_t( s5 ) ) atomicMax( &child->mx[2], mxz );
}

__device__ __forceinline__ uint32_t lvPrefix( const uint32_t* __restrict__ loc, const uint32_t* sums, uint32_t tiles, uint32_t i, uint32_t n ) {
  return i < n ? loc[i] + sums[i / kScanTile] : sums[tiles];
}
// The prefix sums at two positions (the ends of a sweep), both look-ups issued together.  A segment may end at n, where the
// prefix is the grand total: the address is clamped and what it returns is not used.
__device__ __forceinline__ void lvPrefix2( const uint32_t* __restrict__ loc, const uint32_t* sums, uint32_t tiles, uint32_t i0, uint32_t i1, uint32_t n,
                                           uint32_t& r0, uint32_t& r1 ) {
  uint32_t l0 = loc[min( i0, n - 1u )], l1 = loc[min( i1, n - 1u )];
  pin( l0, l1 );
  r0 = i0 < n ? l0 + sums[i0 / kScanTile] : sums[tiles];
  r1 = i1 < n ? l1 + sums[i1 / kScanTile] : sums[tiles];
}

// The position of the element of global rank G among the elements that are NOT of the sweep's class, known to lie in
// [from, to): U( T ) = T * kScanTile - sums[T] such elements precede tile T (sums in LDS), the tile's list holds their offsets.
__device__ __forceinline__ uint32_t lvPartner( const uint16_t* __restrict__ list, const uint32_t* sums, uint32_t from, uint32_t to, uint32_t G ) {
  uint32_t lo = from / kScanTile, hi = ( to - 1u ) / kScanTile;
  while ( lo < hi ) {
    const uint32_t mid = ( lo + hi + 1u ) / 2u;
    if ( mid * kScanTile - sums[mid] <= G )
      lo = mid;
    else
      hi = mid - 1u;
  }
  return lo * kScanTile + list[size_t( lo ) * kScanTile + ( G - ( lo * kScanTile - sums[lo] ) )];
}

// tree-order arrays start as the input order; the root's tight range on the way (one report per workgroup).  The root record
// itself (lvA[0], counts[0], nodeCount) is set up by the memset + lvRootKernel queued before this launch.
__global__ __launch_bounds__( kBlock ) void lvInitKernel( BuildArgs a ) {
  __shared__ int blockRange[6 * kWaves];
  const uint32_t n = a.n, gsize = gridDim.x * blockDim.x;
  const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int mnx = 0x7FFFFFFF, mny = mnx, mnz = mnx, mxx = int( 0x80000000 ), mxy = mxx, mxz = mxx;
  for ( uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsize ) {
    const Pt p = a.pts[i];
    a.P[i]     = p;
    a.perm[i]  = i;
    a.seg[i]   = 0;
    mnx = min( mnx, int( p.x ) ), mny = min( mny, int( p.y ) ), mnz = min( mnz, int( p.z ) );
    mxx = max( mxx, int( p.x ) ), mxy = max( mxy, int( p.y ) ), mxz = max( mxz, int( p.z ) );
  }
  mnx = waveMin( mnx ), mny = waveMin( mny ), mnz = waveMin( mnz );
  mxx = waveMax( mxx ), mxy = waveMax( mxy ), mxz = waveMax( mxz );
  if ( lane == 0 ) {
    int* w = blockRange + 6 * wave;
    w[0] = mnx, w[1] = mny, w[2] = mnz, w[3] = mxx, w[4] = mxy, w[5] = mxz;
  }
  __syncthreads();
  if ( threadIdx.x < 6 ) {
    int v = blockRange[threadIdx.x];
    for ( int w = 1; w < kWaves; ++w ) v = threadIdx.x < 3 ? min( v, blockRange[6 * w + threadIdx.x] ) : max( v, blockRange[6 * w + threadIdx.x] );
    int32_t* slot = threadIdx.x < 3 ? &a.lvA[0].mn[threadIdx.x] : &a.lvA[0].mx[threadIdx.x - 3];
    if ( threadIdx.x < 3 ) {
      if ( v < loadStaleOk( slot ) ) atomicMin( slot, v );
    } else {
      if ( v > loadStaleOk( slot ) ) atomicMax( slot, v );
    }
  }
}
__global__ void lvRootKernel( BuildArgs a ) {  // (one workgroup of 128: it also clears the counters -- one launch instead of a memset + this)
  if ( threadIdx.x < kMaxLevels + 16 ) a.counts[threadIdx.x] = 0;
  __syncthreads();
  if ( threadIdx.x != 0 ) return;
  LvSeg r{};
  r.begin = 0, r.end = a.n, r.node = 0, r.parent = kNone;
  for ( int d = 0; d < 3; ++d ) r.mn[d] = 0x7FFFFFFF, r.mx[d] = int32_t( 0x80000000 );
  a.lvA[0]     = r;
  a.counts[0]  = 1;
  *a.nodeCount = 1;  // node 0 = the root
}

// Once per level, one workgroup: every segment of the level reports its tight range to its parent's node record (divlow /
// divhigh), and is a leaf, a piece for pieceKernel, or splits -- then its rule, and (a prefix sum over the segments that split)
// the slots and node ids of its children.
constexpr int kDecideThreads = 1024;
constexpr int kDecideRng     = 2000;  // segments of a level whose ranges are folded in LDS (48 KB)
__global__ __launch_bounds__( kDecideThreads ) void lvDecideKernel( BuildArgs a, uint32_t level ) {
  __shared__ uint32_t waveTot[kDecideThreads / 64];
  __shared__ uint32_t sCarry;
  __shared__ int32_t  sRng[kDecideRng][6];
  LvSeg*         cur   = ( level & 1 ) ? a.lvB : a.lvA;
  const uint32_t count = a.counts[level], nodeBase = *a.nodeCount;
  const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ( threadIdx.x == 0 ) sCarry = 0;
  // What the workgroups of the landing pass found for the children of the segment they sat in (one record per workgroup and
  // round, in position order: records of one segment are neighbours) is folded HERE -- thousands of workgroups reporting to the
  // same twelve words queue up for ~ 100 us near the root, and so do a few hundred atomics of this one workgroup (they are
  // carried out past the L2, one after the other): segmented wavefront reductions, then LDS atomics into a table of the
  // level's segments; only a level of more than kDecideRng segments goes through global memory.
  const bool inLds = level > 0 && count <= a.decideRng;
  if ( inLds ) {
    for ( uint32_t t = threadIdx.x; t < count * 6u; t += kDecideThreads ) sRng[t / 6u][t % 6u] = ( t % 6u ) < 3u ? 0x7FFFFFFF : int32_t( 0x80000000 );
    __syncthreads();
  }
  if ( level > 0 ) {
    const uint32_t nPart = ( a.n + uint32_t( kLandBlock * kLandRounds ) - 1u ) / uint32_t( kLandBlock * kLandRounds );
    for ( uint32_t base = 0; base < nPart; base += kDecideThreads ) {  // (uniform over the workgroup)
      const uint32_t t = base + threadIdx.x;
      LvPartial      pt;
      pt.slot = kNone;
      if ( t < nPart ) pt = a.partial[t];
#pragma unroll
      for ( int c = 0; c < 2; ++c ) {
        uint32_t A = pt.v[3 * c], B = pt.v[3 * c + 1], C = pt.v[3 * c + 2];
        if ( waveSegMinMaxPacked( pt.slot == kNone ? kNoKey : pt.slot, A, B, C, lane ) ) {
          if ( inLds ) {
            int32_t* r = sRng[pt.slot + c];
            ldsMin( &r[0], pkLo( A ) ), ldsMin( &r[1], pkHi( A ) ), ldsMin( &r[2], pkLo( C ) );
            ldsMax( &r[3], pkLo( B ) ), ldsMax( &r[4], pkHi( B ) ), ldsMax( &r[5], ~pkHi( C ) );
          } else {
            lvReport( cur + pt.slot + c, pkLo( A ), pkHi( A ), pkLo( C ), pkLo( B ), pkHi( B ), ~pkHi( C ) );
          }
        }
      }
    }
    // (global atomics are carried out at agent scope, i.e. past this XCD's L2: once acknowledged, the agent-scope loads below
    //  see them -- a release fence here would write the whole L2 back, tens of microseconds)
    if ( !inLds ) asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
  }
  __syncthreads();
  for ( uint32_t base = 0; base < count; base += kDecideThreads ) {
    const uint32_t s     = base + threadIdx.x;
    uint32_t       split = 0;
    LvSeg*         q     = cur + s;
    if ( s < count ) {
      const bool root = q->parent == kNone;
      int32_t    mn[3], mx[3], lo[3], hi[3];
#pragma unroll
      for ( int d = 0; d < 3; ++d ) {
        mn[d] = __hip_atomic_load( &q->mn[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );  // (what was reported directly)
        mx[d] = __hip_atomic_load( &q->mx[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
        if ( inLds ) mn[d] = min( mn[d], sRng[s][d] ), mx[d] = max( mx[d], sRng[s][3 + d] );
        lo[d] = root ? mn[d] : int32_t( q->lo[d] );
        hi[d] = root ? mx[d] : int32_t( q->hi[d] );
      }
      if ( root ) {
        for ( int d = 0; d < 3; ++d ) a.rootBox[d] = mn[d], a.rootBox[3 + d] = mx[d];
      } else {
        const int pd = q->pdim;
        if ( q->side == 0 )
          a.nodes[q->parent].divlow = int16_t( pd == 0 ? mx[0] : ( pd == 1 ? mx[1] : mx[2] ) );
        else
          a.nodes[q->parent].divhigh = int16_t( pd == 0 ? mn[0] : ( pd == 1 ? mn[1] : mn[2] ) );
      }
      const uint32_t cnt = q->end - q->begin;
      if ( cnt <= uint32_t( kLeafMax ) ) {
        KdNode nd;
        nd.a = int32_t( q->begin ), nd.b = int32_t( q->end ), nd.divlow = nd.divhigh = 0, nd.dim = -1;
        a.nodes[q->node] = nd;
      } else if ( cnt <= a.retireMax ) {  // the rest of this subtree is built in LDS
        RetiredSeg r;
        r.begin = q->begin, r.end = q->end, r.node = q->node, r.level = level;
        r.root  = root ? 1 : 0;
        for ( int d = 0; d < 3; ++d ) r.lo[d] = q->lo[d], r.hi[d] = q->hi[d];
        a.retired[atomicAdd( a.retiredCount, 1u )] = r;
      } else if ( cnt <= a.hugeMax ) {  // one workgroup cuts it into pieces where it lies (hugeSegmentsKernel)
        HugeSeg r;
        r.begin = q->begin, r.end = q->end, r.node = q->node, r.level = level;
        r.root  = root ? 1 : 0;
        for ( int d = 0; d < 3; ++d ) r.lo[d] = q->lo[d], r.hi[d] = q->hi[d], r.mn[d] = mn[d], r.mx[d] = mx[d];
        a.huge[atomicAdd( a.hugeCount, 1u )] = r;
      } else {
        const int32_t maxSpan = max( hi[0] - lo[0], max( hi[1] - lo[1], hi[2] - lo[2] ) );
        const double  limit   = ( 1.0 - 0.00001 ) * double( maxSpan );
        int           dim     = 0;
        int32_t       best    = -1;
        if ( double( hi[0] - lo[0] ) > limit && mx[0] - mn[0] > best ) best = mx[0] - mn[0], dim = 0;
        if ( double( hi[1] - lo[1] ) > limit && mx[1] - mn[1] > best ) best = mx[1] - mn[1], dim = 1;
        if ( double( hi[2] - lo[2] ) > limit && mx[2] - mn[2] > best ) best = mx[2] - mn[2], dim = 2;
        const int32_t l = dim == 0 ? lo[0] : ( dim == 1 ? lo[1] : lo[2] ), h = dim == 0 ? hi[0] : ( dim == 1 ? hi[1] : hi[2] );
        const int32_t lowest = dim == 0 ? mn[0] : ( dim == 1 ? mn[1] : mn[2] ), highest = dim == 0 ? mx[0] : ( dim == 1 ? mx[1] : mx[2] );
        const int32_t cut = min( max( ( l + h ) / 2, lowest ), highest );
        q->cutInfo = ( uint32_t( cut ) & 0xFFFFu ) | ( uint32_t( dim ) << 16 ) | ( 1u << 24 );
        if ( root )
          for ( int d = 0; d < 3; ++d ) q->lo[d] = int16_t( mn[d] ), q->hi[d] = int16_t( mx[d] );  // (its children inherit the tight box)
        split = 1;
      }
      if ( !split ) q->cutInfo = 0;
    }
    const uint32_t inc = waveInclusive( split, lane );
    if ( lane == 63 ) waveTot[wave] = inc;
    __syncthreads();
    uint32_t before = sCarry, all = 0;
    for ( int w = 0; w < kDecideThreads / 64; ++w ) {
      all += waveTot[w];
      before += w < wave ? waveTot[w] : 0u;
    }
    const uint32_t rank = before + inc - split;
    if ( split ) q->slot = 2u * rank, q->childNode = nodeBase + 2u * rank;
    __syncthreads();
    if ( threadIdx.x == 0 ) sCarry += all;
    __syncthreads();
  }
  if ( threadIdx.x == 0 ) {
    a.counts[level + 1] = 2u * sCarry;
    *a.nodeCount        = nodeBase + 2u * sCarry;
  }
  if ( a.hostSmall ) {  // the last decide pass of a batch of levels: the counter block as the host will want it (one workgroup: it is all ours)
    if ( threadIdx.x == 0 ) __threadfence();
    __syncthreads();
    if ( threadIdx.x < kMaxLevels + 16 ) a.hostSmall[threadIdx.x] = __hip_atomic_load( &a.counts[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
  }
}

// flags of a sweep (FIRST: ">= cut" over the whole segment; second: "> cut" from the first sweep's edge on), their prefix sums
// (tile-local + tile totals scanned by the block that finishes last), and the tile's list of the positions NOT of the class
template <bool FIRST>
__global__ __launch_bounds__( kBlock ) void lvFlagKernel( BuildArgs a, uint32_t level ) {
  __shared__ uint32_t waveTot[kWaves];
  const uint32_t n = a.n, tiles = a.tiles;
  LvSeg*         cur   = ( level & 1 ) ? a.lvB : a.lvA;
  LvSeg*         next  = ( level & 1 ) ? a.lvA : a.lvB;
  const uint32_t count = a.counts[level];
  uint32_t*      loc   = FIRST ? a.loc1 : a.loc2;
  uint32_t*      tile  = FIRST ? a.tile1 : a.tile2;
  if ( !FIRST ) {  // the children's ranges start empty (the landing pass gathers them)
    for ( uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < count; s += gridDim.x * blockDim.x ) {
      const LvSeg* q  = cur + s;
      uint32_t     ci = q->cutInfo, slot = q->slot;  // (one batch; the stores below cannot make the compiler read them again)
      pin( ci, slot );
      if ( !( ci >> 24 ) ) continue;
      for ( int c = 0; c < 2; ++c ) {  // (the words of LvSeg::mn / mx: a row and a half)
        uint32_t* w = reinterpret_cast<uint32_t*>( next[slot + c].mn );
        *reinterpret_cast<Words4*>( w )     = Words4{0x7FFFFFFFu, 0x7FFFFFFFu, 0x7FFFFFFFu, 0x80000000u};
        *reinterpret_cast<Words2*>( w + 4 ) = Words2{0x80000000u, 0x80000000u};
      }
    }
  }
  // A thread owns 8 consecutive positions (32 bytes of seg and loc, 64 of P, all 16-byte aligned: the arrays start on 32-byte
  // boundaries and are padded to whole groups).  Two round trips per tile: the 8 segment ids; then, together, the cut word(s)
  // of the 8 records and the 8 points.  Positions at or beyond n and retired positions read record 0 / point 0 instead (always
  // there) and what comes back is not used.
  for ( uint32_t t = blockIdx.x; t < tiles; t += gridDim.x ) {
    const uint32_t base = t * kScanTile + threadIdx.x * 8;
    uint32_t       run = 0, flags = 0, liveAt = 0;  // (bit k: position base + k carries the class flag / lies in a segment)
    Words4           sA = Words4{kNone, kNone, kNone, kNone}, sB = sA;
    if ( base < n ) sA = *reinterpret_cast<const Words4*>( a.seg + base );
    if ( base + 4 < n ) sB = *reinterpret_cast<const Words4*>( a.seg + base + 4 );
    pin( sA, sB );
    uint32_t sg[8] = {sA.x, sA.y, sA.z, sA.w, sB.x, sB.y, sB.z, sB.w};
    uint32_t ci[8], e1[8];
    Words4     pp[4];
#pragma unroll
    for ( int k = 0; k < 8; ++k ) {
      if ( base + k >= n ) sg[k] = kNone;  // (the padding of a group that n cuts holds whatever the pool left there)
      liveAt |= uint32_t( sg[k] != kNone ) << k;
      const LvSeg* q = cur + ( sg[k] != kNone ? sg[k] : 0u );
      if ( FIRST ) {
        ci[k] = q->cutInfo, e1[k] = 0;
      } else {
        const Words2 w = *reinterpret_cast<const Words2*>( &q->cutInfo );  // cutInfo, edge1
        ci[k] = w.x, e1[k] = w.y;
      }
    }
#pragma unroll
    for ( int m = 0; m < 4; ++m ) pp[m] = *reinterpret_cast<const Words4*>( a.P + ( base + 2 * m < n ? base + 2 * m : 0u ) );  // (P has a spare element past n)
#pragma unroll
    for ( int k = 0; k < 8; ++k ) pin( ci[k] ), pin( e1[k] );
    pin( pp[0], pp[1], pp[2], pp[3] );
#pragma unroll
    for ( int k = 0; k < 8; ++k ) {
      const uint32_t i  = base + k;
      const uint32_t lw = ( k & 1 ) ? pp[k / 2].z : pp[k / 2].x, hw = ( k & 1 ) ? pp[k / 2].w : pp[k / 2].y;  // x | y << 16, z | w << 16
      const int      dim = int( ( ci[k] >> 16 ) & 0xFFu );
      const int32_t  c = int32_t( int16_t( ci[k] & 0xFFFFu ) );
      const int32_t  x = dim == 0 ? int32_t( int16_t( lw & 0xFFFFu ) ) : ( dim == 1 ? int32_t( int16_t( lw >> 16 ) ) : int32_t( int16_t( hw & 0xFFFFu ) ) );
      const bool     live = ( ( liveAt >> k ) & 1u ) != 0 && ( ci[k] >> 24 ) != 0;
      const uint32_t f    = live ? ( FIRST ? uint32_t( x >= c ) : uint32_t( i >= e1[k] && x > c ) ) : 0u;
      flags |= f << k;
      run += f;
    }
    uint32_t offset = blockExclusive<kWaves>( run, waveTot );
    uint32_t at[8];
#pragma unroll
    for ( int k = 0; k < 8; ++k ) {
      at[k] = offset;
      const uint32_t f = ( flags >> k ) & 1u;
      if ( base + k < n && !f ) a.list[size_t( t ) * kScanTile + ( threadIdx.x * 8 + k - offset )] = uint16_t( threadIdx.x * 8 + k );
      offset += f;
    }
    if ( base < n ) *reinterpret_cast<Words4*>( loc + base ) = Words4{at[0], at[1], at[2], at[3]};            // (into the padding where n cuts
    if ( base + 4 < n ) *reinterpret_cast<Words4*>( loc + base + 4 ) = Words4{at[4], at[5], at[6], at[7]};    //  the group: never read)
    if ( threadIdx.x == kBlock - 1 ) tile[t] = offset;  // (the RAW total: the swap passes scan the totals themselves, in LDS)
    __syncthreads();
  }
}

// The tile totals of a flag pass (raw, in global memory) -> their exclusive prefix sums in LDS, sums[tiles] = the grand total.
// Every workgroup of a swap pass does this for itself: a few hundred words, one LDS scan -- instead of the flag pass ending in
// a ticket, a hand-off to the workgroup that finishes last and ITS scan, with the whole chip waiting.
template <int BLOCK>
__device__ __forceinline__ void lvLoadSums( uint32_t* sums, const uint32_t* __restrict__ raw, uint32_t tiles ) {
  __shared__ uint32_t waveTot[BLOCK / 64];
  uint32_t            carry = 0;
  for ( uint32_t base = 0; base < tiles; base += BLOCK ) {
    const uint32_t i   = base + threadIdx.x;
    const uint32_t v   = i < tiles ? raw[i] : 0u;
    uint32_t       all;
    const uint32_t offset = carry + blockExclusive<BLOCK / 64>( v, waveTot, all );
    if ( i < tiles ) sums[i] = offset;
    carry += all;
    __syncthreads();
  }
  if ( threadIdx.x == 0 ) sums[tiles] = carry;
  __syncthreads();
}

// first sweep: the misplaced left-hand elements (">= cut" before the edge) swap with the misplaced right-hand element of the
// same rank counted from the segment's end
__global__ __launch_bounds__( kBlock ) void lvSwapOneKernel( BuildArgs a, uint32_t level ) {
  extern __shared__ uint32_t lvSums[];  // [tiles + 1]
  const uint32_t n = a.n, tiles = a.tiles;
  const uint32_t gsize = gridDim.x * blockDim.x;
  LvSeg*         cur = ( level & 1 ) ? a.lvB : a.lvA;
  lvLoadSums<kBlock>( lvSums, a.tile1, tiles );
  for ( uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsize ) {
    const uint32_t s = a.seg[i];
    if ( s == kNone ) continue;
    LvSeg*         q  = cur + s;
    const uint32_t ci = q->cutInfo;
    if ( !( ci >> 24 ) ) continue;
    const uint32_t b = q->begin, e = q->end;
    const Pt       pi = a.P[i];
    const uint32_t li = a.loc1[i];
    const uint32_t rb = lvPrefix( a.loc1, lvSums, tiles, b, n ), re = lvPrefix( a.loc1, lvSums, tiles, e, n );
    const uint32_t edge = b + ( ( e - b ) - ( re - rb ) );
    if ( i == b ) q->edge1 = edge;
    if ( i >= edge || coordOf( pi, int( ( ci >> 16 ) & 0xFFu ) ) < int32_t( int16_t( ci & 0xFFFFu ) ) ) continue;
    const uint32_t r  = li + lvSums[i / kScanTile] - rb;
    const uint32_t j  = lvPartner( a.list, lvSums, edge, e, ( e - re ) - 1u - r );
    const Pt       pj = a.P[j];
    a.P[i]            = pj;
    a.P[j]            = pi;
    const uint32_t u  = a.perm[i];
    a.perm[i]         = a.perm[j];
    a.perm[j]         = u;
  }
}

// second sweep's swaps, and the landing: every position learns its child (its segment of the next level), the children's
// tight ranges are gathered, the thread on a segment's first position writes the children and the node record
__global__ __launch_bounds__( kLandBlock ) void lvSwapTwoKernel( BuildArgs a, uint32_t level ) {
  extern __shared__ uint32_t lvSums[];  // [tiles + 1]
  const uint32_t n = a.n, tiles = a.tiles;
  const int      lane  = threadIdx.x & 63;
  LvSeg*         cur  = ( level & 1 ) ? a.lvB : a.lvA;
  LvSeg*         next = ( level & 1 ) ? a.lvA : a.lvB;
  lvLoadSums<kLandBlock>( lvSums, a.tile2, tiles );
  const uint32_t nRound = ( n + uint32_t( kLandBlock ) - 1u ) & ~( uint32_t( kLandBlock ) - 1u );
  __shared__ uint32_t blockSeg;
  __shared__ uint32_t red[kLandBlock / 64][6];
  __shared__ uint32_t accV[6], accSlot;  // what the rounds of this pass have found so far for the children of ONE segment
  const int wave = threadIdx.x >> 6;
  constexpr uint32_t kChunk = uint32_t( kLandBlock ) * kLandRounds;  // a workgroup lands kLandRounds consecutive rounds and leaves one record
  for ( uint32_t c0 = blockIdx.x * kChunk; c0 < nRound; c0 += gridDim.x * kChunk ) {
  if ( threadIdx.x == 0 ) accSlot = kNone;  // (ordered before its first use by the barriers of the round)
  for ( uint32_t i0 = c0; i0 < min( c0 + kChunk, nRound ); i0 += kLandBlock ) {  // (uniform per workgroup: it reduces together)
    const uint32_t i   = i0 + threadIdx.x;
    uint32_t       key = kNoKey;  // the child the element that ENDS at position i belongs to
    uint32_t       A = pk2( 0x7FFF, 0x7FFF ), B = pk2( -0x8000, -0x8000 ), C = pk2( 0x7FFF, 0x7FFF );      // ... that element
    uint32_t       A2 = A, B2 = B, C2 = C;  // the element a swap of this thread has moved away (always into the RIGHT child: mid <= edge2)
    bool           moved = false;
    uint32_t       s = kNone, slot = 0;
    if ( i < n ) {
      // the chain of a position: seg -> { record rows 0, 1, 2, P[i], loc2[i], perm[i] } -> { loc2[edge1], loc2[end] } -> list ->
      // { P[j], perm[j] }.  Row 2 (the loose box) is only used by the thread on the segment's first position; which one that is
      // comes with row 0, so everybody asks for it in the same batch (the lanes of a segment ask for the same 16 bytes).
      s = a.seg[i];
      Words2     pw;
      uint32_t li, u;
      uint32_t to = kNone;
      if ( s != kNone ) {
        LvSeg* q  = cur + s;
        Words4   r0 = lvRow( q, 0 ), r1 = lvRow( q, 1 ), r2 = lvRow( q, 2 );
        pw = *reinterpret_cast<const Words2*>( a.P + i ), li = a.loc2[i], u = a.perm[i];
        pin( r0, r1, r2, pw, li, u );
        const uint32_t ci = r0.z;
        if ( ci >> 24 ) {
          const uint32_t b = r0.x, e = r0.y, e1 = r0.w;
          slot               = r1.x;
          const int      dim = int( ( ci >> 16 ) & 0xFFu );
          const int32_t  cut = int32_t( int16_t( ci & 0xFFFFu ) );
          uint32_t       rb, re;
          lvPrefix2( a.loc2, lvSums, tiles, e1, e, n, rb, re );
          const uint32_t e2   = e1 + ( ( e - e1 ) - ( re - rb ) );
          const uint32_t cnt  = e - b, half = cnt / 2, lim1 = e1 - b, lim2 = e2 - b;
          const uint32_t idx  = lim1 > half ? lim1 : ( lim2 < half ? lim2 : half );
          const uint32_t mid  = b + idx;
          if ( i == b ) {  // the children (their ranges are being gathered by everybody: not touched here) and the node record
            const uint32_t childNode = r1.y, node = r1.z;
            KdNode         nd;
            nd.a = int32_t( childNode ), nd.b = int32_t( childNode + 1u ), nd.divlow = nd.divhigh = 0, nd.dim = dim;
            a.nodes[node] = nd;
            // both children built in registers from the parent's rows and stored as whole rows 0 .. 2: the left one takes the cut
            // as hi[dim], the right one as lo[dim] (row 2 = lo[0] lo[1] | lo[2] hi[0] | hi[1] hi[2] | side, pdim, unused)
            const uint32_t c16 = uint32_t( cut ) & 0xFFFFu;
            Words4           left = r2, right = r2;
            if ( dim == 0 ) left.y = ( r2.y & 0x0000FFFFu ) | ( c16 << 16 ), right.x = ( r2.x & 0xFFFF0000u ) | c16;
            if ( dim == 1 ) left.z = ( r2.z & 0xFFFF0000u ) | c16, right.x = ( r2.x & 0x0000FFFFu ) | ( c16 << 16 );
            if ( dim == 2 ) left.z = ( r2.z & 0x0000FFFFu ) | ( c16 << 16 ), right.y = ( r2.y & 0xFFFF0000u ) | c16;
            left.w = uint32_t( dim ) << 8, right.w = 1u | ( uint32_t( dim ) << 8 );
            LvSeg* ch = next + slot;
            lvStoreRow( ch, 0, Words4{b, mid, 0u, 0u} );
            lvStoreRow( ch, 1, Words4{0u, 0u, childNode, node} );
            lvStoreRow( ch, 2, left );
            lvStoreRow( ch + 1, 0, Words4{mid, e, 0u, 0u} );
            lvStoreRow( ch + 1, 1, Words4{0u, 0u, childNode + 1u, node} );
            lvStoreRow( ch + 1, 2, right );
          }
          const int32_t x = ptCoord( pw, dim );
          to              = slot + ( i >= mid ? 1u : 0u );
          key             = to;
          if ( i >= e1 && i < e2 && x > cut ) {  // misplaced on the left of the second sweep: swap; what moves away lands right of mid
            const uint32_t r  = li + lvSums[i / kScanTile] - rb;
            const uint32_t j  = lvPartner( a.list, lvSums, e2, e, ( e - re ) - 1u - r );
            Words2           pj = *reinterpret_cast<const Words2*>( a.P + j );
            uint32_t       uj = a.perm[j];
            pin( pj, uj );
            *reinterpret_cast<Words2*>( a.P + i ) = pj;
            *reinterpret_cast<Words2*>( a.P + j ) = pw;
            a.perm[i]                            = uj;
            a.perm[j]                            = u;
            moved                                = true;
            A2 = pw.x, B2 = A2, C2 = pk2( ptCoord( pw, 2 ), ~ptCoord( pw, 2 ) );
            pw = pj;
          }
          // (misplaced on the right of the second sweep: the partner swaps and reports what lands here -- this lane keeps the
          //  run of its child together and adds nothing; if the swap has happened already it sees the element that landed)
          if ( !( i >= e2 && x <= cut ) ) A = pw.x, B = A, C = pk2( ptCoord( pw, 2 ), ~ptCoord( pw, 2 ) );
        }
        a.seg[i] = to;
      }
    }
    // Near the root a whole workgroup sits inside one segment: then it reduces for the two children in registers / LDS and
    // reports ONCE per child -- otherwise thousands of wavefronts queue up on the same six words of a handful of records.
    if ( threadIdx.x == 0 ) blockSeg = s;
    __syncthreads();
    const bool uniform = __syncthreads_and( s == blockSeg ) != 0;
    if ( uniform ) {
      const bool anything = __syncthreads_or( key != kNoKey ) != 0;
      if ( anything ) {  // (one segment, and it splits: slot is the same for every lane)
        uint32_t v[6];
        const bool right = key != kNoKey && key != slot;
        v[0] = right || key == kNoKey ? pk2( 0x7FFF, 0x7FFF ) : A, v[1] = right || key == kNoKey ? pk2( -0x8000, -0x8000 ) : B,
        v[2] = right || key == kNoKey ? pk2( 0x7FFF, 0x7FFF ) : C;
        v[3] = pkMin( right ? A : pk2( 0x7FFF, 0x7FFF ), A2 ), v[4] = pkMax( right ? B : pk2( -0x8000, -0x8000 ), B2 ),
        v[5] = pkMin( right ? C : pk2( 0x7FFF, 0x7FFF ), C2 );
#pragma unroll
        for ( int k = 0; k < 6; ++k ) v[k] = ( k % 3 ) == 1 ? waveReduce( v[k], pkMax ) : waveReduce( v[k], pkMin );
        if ( lane == 0 )
          for ( int k = 0; k < 6; ++k ) red[wave][k] = v[k];
        __syncthreads();
        if ( threadIdx.x == 0 ) {  // merged into the pass' record (in position order: lvDecideKernel folds the records of all passes)
          uint32_t x[6];
          for ( int k = 0; k < 6; ++k ) {
            x[k] = red[0][k];
            for ( int w = 1; w < kLandBlock / 64; ++w ) x[k] = ( k % 3 ) == 1 ? pkMax( x[k], red[w][k] ) : pkMin( x[k], red[w][k] );
          }
          if ( accSlot != kNone && accSlot != slot ) {  // the earlier rounds sat in another segment: that one reports for itself
            for ( int c = 0; c < 2; ++c )
              lvReport( next + accSlot + c, pkLo( accV[3 * c] ), pkHi( accV[3 * c] ), pkLo( accV[3 * c + 2] ), pkLo( accV[3 * c + 1] ), pkHi( accV[3 * c + 1] ),
                        ~pkHi( accV[3 * c + 2] ) );
            accSlot = kNone;
          }
          for ( int k = 0; k < 6; ++k ) accV[k] = accSlot == kNone ? x[k] : ( ( k % 3 ) == 1 ? pkMax( accV[k], x[k] ) : pkMin( accV[k], x[k] ) );
          accSlot = slot;
        }
      }
      __syncthreads();
      continue;
    }
    if ( moved ) lvReport( next + slot + 1u, pkLo( A2 ), pkHi( A2 ), pkLo( C2 ), pkLo( A2 ), pkHi( A2 ), pkLo( C2 ) );
    if ( waveSegMinMaxPacked( key, A, B, C, lane ) )
      lvReport( next + key, pkLo( A ), pkHi( A ), pkLo( C ), pkLo( B ), pkHi( B ), ~pkHi( C ) );
  }
  __syncthreads();
  if ( threadIdx.x == 0 ) {
    LvPartial pt;
    pt.slot = accSlot, pt.unused = 0;
    for ( int k = 0; k < 6; ++k ) pt.v[k] = accV[k];
    a.partial[c0 / kChunk] = pt;
  }
  __syncthreads();
  }
}

constexpr size_t kPieceLdsBytes = size_t( kPieceMax ) * ( sizeof( Pt ) + 4 + 2 + 2 + 2 ) + 16 + 2 * size_t( kPieceRecs ) * sizeof( PieceRec );

constexpr int kPiecePer = 4;  // positions per thread: kPieceMax / 4 = 1 024 threads (eight per thread, 512 threads, measured and dropped)
template <bool PROFILE = false>
__global__ __launch_bounds__( kPieceMax / kPiecePer ) void pieceKernel( BuildArgs a ) {
  unsigned long long profLast = 0, prof[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define PIECE_MARK( k )                                        \
  if ( PROFILE && threadIdx.x == 0 ) {                         \
    const unsigned long long now_ = wall_clock64();            \
    prof[k] += now_ - profLast, profLast = now_;               \
  }
  constexpr int K = kPiecePer, THREADS = kPieceMax / K, WAVES = THREADS / 64;
  extern __shared__ __align__( 16 ) unsigned char pieceLds[];
  Pt*       P     = reinterpret_cast<Pt*>( pieceLds );                       // [kPieceMax] the piece's points
  uint32_t* perm  = reinterpret_cast<uint32_t*>( P + kPieceMax );            // [kPieceMax]
  uint16_t* pre   = reinterpret_cast<uint16_t*>( perm + kPieceMax );         // [kPieceMax + 8] exclusive prefix of a sweep's class flag
  uint16_t* lst   = pre + kPieceMax + 8;                                     // [kPieceMax] misplaced right-hand positions by rank
  uint16_t* segOf = lst + kPieceMax;                                         // [kPieceMax] record of a position (kNoRec: settled)
  PieceRec* recs  = reinterpret_cast<PieceRec*>( segOf + kPieceMax );        // [2][kPieceRecs]
  __shared__ __align__( 16 ) uint32_t sWave[2][WAVES];
  __shared__ uint32_t sCount[2], sNodeBase, sDepth;
  const int      lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t total = *a.retiredCount;
  const uint32_t p0    = uint32_t( tid ) * K;
  // (measured and dropped: largest pieces first -- every workgroup ranking the list for itself; 302 against 291 us: the launch is
  //  bound by the sum of the pieces' work over the CUs, not by a late large piece)
  for ( uint32_t s = blockIdx.x; s < total; s += gridDim.x ) {  // (uniform over the workgroup)
    const RetiredSeg seg = a.retired[s];
    const uint32_t   cnt = seg.end - seg.begin;
    uint32_t idPending   = 0;  // thread 0: node ids of the children of the coming depth's records (a returning atomic in flight)
    if ( tid == 0 ) idPending = atomicAdd( a.nodeCount, 2u );
    pieceBarrier();  // (the previous piece's stores have read the arrays)
    for ( uint32_t i = tid; i < uint32_t( kPieceMax ); i += THREADS ) {
      if ( i < cnt ) {
        P[i]     = a.P[seg.begin + i];
        perm[i]  = a.perm[seg.begin + i];
        segOf[i] = 0;
      } else {
        segOf[i] = kNoRec;
      }
    }
    if ( tid == 0 ) {
      PieceRec r{};
      r.begin = 0, r.end = uint16_t( cnt ), r.node = seg.node;
      for ( int d = 0; d < 3; ++d ) r.lo[d] = seg.lo[d], r.hi[d] = seg.hi[d], r.mn[d] = 0x7FFFFFFF, r.mx[d] = int32_t( 0x80000000 );
      recs[0]   = r;
      sCount[0] = 1, sCount[1] = 0, sDepth = 0;
    }
    pieceBarrier();
    {  // tight range of the piece's root
      uint32_t A = pk2( 0x7FFF, 0x7FFF ), B = pk2( -0x8000, -0x8000 ), C = pk2( 0x7FFF, 0x7FFF );
      bool     any = false;
#pragma unroll
      for ( int k = 0; k < K; ++k ) {
        const uint32_t p = p0 + k;
        if ( p < cnt ) {
          const Pt x = P[p];
          A = pkMin( A, pk2( x.x, x.y ) ), B = pkMax( B, pk2( x.x, x.y ) ), C = pkMin( C, pk2( x.z, ~int( x.z ) ) );
          any = true;
        }
      }
      if ( waveSegMinMaxPacked( any ? 0u : kNoKey, A, B, C, lane ) ) {
        ldsMin( &recs[0].mn[0], pkLo( A ) ), ldsMin( &recs[0].mn[1], pkHi( A ) ), ldsMin( &recs[0].mn[2], pkLo( C ) );
        ldsMax( &recs[0].mx[0], pkLo( B ) ), ldsMax( &recs[0].mx[1], pkHi( B ) ), ldsMax( &recs[0].mx[2], ~pkHi( C ) );
      }
    }
    pieceBarrier();
    if ( seg.root != 0 && tid == 0 ) {  // the root of the whole tree: its loose box is its tight range
      for ( int d = 0; d < 3; ++d ) {
        recs[0].lo[d] = int16_t( recs[0].mn[d] ), recs[0].hi[d] = int16_t( recs[0].mx[d] );
        a.rootBox[d] = recs[0].mn[d], a.rootBox[3 + d] = recs[0].mx[d];
      }
    }
    if ( PROFILE && threadIdx.x == 0 ) profLast = wall_clock64();
    uint32_t deepest  = 0;  // (level of the deepest leaf this thread has written) + 1
    uint32_t prevBase = 0, prevCount = 0;
    int      cur      = 0;
    for ( uint32_t depth = 0;; ++depth ) {
      pieceBarrier();  // (the records of this depth and their ranges are complete; so is sCount[cur])
      PIECE_MARK( 0 )  // landing of the previous depth (or the piece's load)
      const uint32_t nc = sCount[cur];
      PieceRec*      R  = recs + cur * kPieceRecs;
      PieceRec*      RN = recs + ( cur ^ 1 ) * kPieceRecs;
      // ---- the node records of the previous depth (their divlow / divhigh are complete now)
      for ( uint32_t r = tid; r < prevCount; r += THREADS ) {
        const PieceRec* q = RN + r;
        KdNode          nd;
        nd.a = int32_t( prevBase + 2u * r ), nd.b = int32_t( prevBase + 2u * r + 1u ), nd.divlow = int16_t( q->lmax ), nd.divhigh = int16_t( q->rmin ),
        nd.dim = q->dim;
        a.nodes[q->node] = nd;
      }
      if ( nc == 0 ) break;
      if ( seg.level + depth >= uint32_t( kMaxLevels ) - 2u ) {  // deeper than the k-NN traversal stack: refused
        if ( tid == 0 ) atomicMax( a.finishDepth, 0x10000u );
        break;
      }
      // ---- the split rule of every record; node ids of their children
      if ( tid == 0 ) sNodeBase = idPending, sCount[cur ^ 1] = 0;
      for ( uint32_t r = tid; r < nc; r += THREADS ) {
        PieceRec*     q   = R + r;
        const int32_t lo0 = q->lo[0], lo1 = q->lo[1], lo2 = q->lo[2], hi0 = q->hi[0], hi1 = q->hi[1], hi2 = q->hi[2];
        const int32_t mn0 = q->mn[0], mn1 = q->mn[1], mn2 = q->mn[2], mx0 = q->mx[0], mx1 = q->mx[1], mx2 = q->mx[2];
        const int32_t maxSpan = max( hi0 - lo0, max( hi1 - lo1, hi2 - lo2 ) );
        const double  limit   = ( 1.0 - 0.00001 ) * double( maxSpan );
        int           dim     = 0;
        int32_t       best    = -1;
        if ( double( hi0 - lo0 ) > limit && mx0 - mn0 > best ) best = mx0 - mn0, dim = 0;
        if ( double( hi1 - lo1 ) > limit && mx1 - mn1 > best ) best = mx1 - mn1, dim = 1;
        if ( double( hi2 - lo2 ) > limit && mx2 - mn2 > best ) best = mx2 - mn2, dim = 2;
        const int32_t l = dim == 0 ? lo0 : ( dim == 1 ? lo1 : lo2 ), h = dim == 0 ? hi0 : ( dim == 1 ? hi1 : hi2 );
        const int32_t lowest = dim == 0 ? mn0 : ( dim == 1 ? mn1 : mn2 ), highest = dim == 0 ? mx0 : ( dim == 1 ? mx1 : mx2 );
        q->dim = uint8_t( dim ), q->unused0 = 0, q->cut = int16_t( min( max( ( l + h ) / 2, lowest ), highest ) );
      }
      pieceBarrier();
      PIECE_MARK( 1 )  // node records of the previous depth + split rules
      // ---- what this thread's positions belong to (kept in registers for the whole depth).  Settled subtrees are contiguous, so
      //      from the middle depths on whole wavefronts hold nothing but settled positions: they keep the barriers and the two prefix
      //      sums company and skip the rest (waveLive).
      uint32_t rec[K], be[K], dc[K];
      bool     waveLive = true;
      {
        uint16_t raw[K];
        *reinterpret_cast<uint2*>( raw ) = *reinterpret_cast<const uint2*>( segOf + p0 );
        bool same = true, live = false;
#pragma unroll
        for ( int k = 0; k < K; ++k ) rec[k] = raw[k], same = same && raw[k] == raw[0], live = live || raw[k] != kNoRec;
        waveLive = __ballot( live ) != 0ull;
        if ( same ) {
          PieceHot0 h{0, 0};
          if ( rec[0] != kNoRec ) h = *reinterpret_cast<const PieceHot0*>( R + rec[0] );
#pragma unroll
          for ( int k = 0; k < K; ++k ) be[k] = h.be, dc[k] = h.dc;
        } else {
#pragma unroll
          for ( int k = 0; k < K; ++k ) {
            PieceHot0 h{0, 0};
            if ( rec[k] != kNoRec ) h = *reinterpret_cast<const PieceHot0*>( R + rec[k] );
            be[k] = h.be, dc[k] = h.dc;
          }
        }
      }
      // ---- first sweep: class ">= cut", prefix sum
      uint32_t f1 = 0;  // bit k: position p0 + k is of the class
      if ( waveLive ) {
        Pt x[K];
#pragma unroll
        for ( int k = 0; k < K; k += 2 ) *reinterpret_cast<uint4*>( &x[k] ) = *reinterpret_cast<const uint4*>( P + p0 + k );
#pragma unroll
        for ( int k = 0; k < K; ++k ) {
          const int d = int( ( dc[k] >> 16 ) & 0xFFu ), c = int( int16_t( dc[k] & 0xFFFFu ) );
          const int v = int( int16_t( __builtin_bit_cast( uint64_t, x[k] ) >> ( 16 * d ) ) );  // (a shift, not a three-way select: that one became an indexed load from the stack)
          if ( rec[k] != kNoRec && v >= c ) f1 |= 1u << k;
        }
      }
      uint32_t preA[K + 1];  // prefix at p0 .. p0 + K
      {
        uint32_t at = pieceScan<WAVES>( uint32_t( __popc( f1 ) ), sWave[0] );
        uint16_t out[K];
#pragma unroll
        for ( int k = 0; k < K; ++k ) preA[k] = at, out[k] = uint16_t( at ), at += ( f1 >> k ) & 1u;
        preA[K] = at;
        *reinterpret_cast<uint2*>( pre + p0 ) = *reinterpret_cast<const uint2*>( out );
        if ( tid == THREADS - 1 ) pre[kPieceMax] = uint16_t( at );
      }
      pieceBarrier();
      PIECE_MARK( 2)  // first flags + prefix sum
      // ---- the misplaced right-hand elements ("< cut" beyond the edge) publish their position by rank from the right
      uint32_t edge1[K], rb1[K];
#pragma unroll
      for ( int k = 0; k < K; ++k ) {
        edge1[k] = rb1[k] = 0;
        if ( !waveLive || rec[k] == kNoRec ) continue;
        if ( k > 0 && rec[k] == rec[k - 1] ) {
          edge1[k] = edge1[k - 1], rb1[k] = rb1[k - 1];
        } else {
          const uint32_t b = be[k] & 0xFFFFu, e = be[k] >> 16, rb = pre[b], re = pre[e];
          edge1[k] = b + ( ( e - b ) - ( re - rb ) ), rb1[k] = rb | ( re << 16 );
        }
        const uint32_t p = p0 + k, b = be[k] & 0xFFFFu, e = be[k] >> 16;
        if ( p >= edge1[k] && !( ( f1 >> k ) & 1u ) ) lst[b + ( ( e - p - 1u ) - ( ( rb1[k] >> 16 ) - preA[k + 1] ) )] = uint16_t( p );
        if ( p == b ) *reinterpret_cast<uint32_t*>( &R[rec[k]].edge1 ) = edge1[k] | ( ( rb1[k] & 0xFFFFu ) << 16 );
      }
      pieceBarrier();
      PIECE_MARK( 3)  // first publish
      // ---- ... and the misplaced left-hand elements (">= cut" before the edge) swap with the entry of their rank from the left
#pragma unroll
      for ( int k = 0; k < K; ++k ) {
        const uint32_t p = p0 + k;
        if ( waveLive && rec[k] != kNoRec && p < edge1[k] && ( ( f1 >> k ) & 1u ) ) {
          const uint32_t j  = lst[( be[k] & 0xFFFFu ) + ( preA[k] - ( rb1[k] & 0xFFFFu ) )];
          const Pt       px = P[p], pj = P[j];
          const uint32_t ip = perm[p], ij = perm[j];
          P[p] = pj, P[j] = px, perm[p] = ij, perm[j] = ip;
        }
      }
      pieceBarrier();
      PIECE_MARK( 4)  // first swaps
      // ---- second sweep on [edge1, end): class "> cut", prefix sum
      uint32_t f2 = 0;
      if ( waveLive ) {
        Pt x[K];
#pragma unroll
        for ( int k = 0; k < K; k += 2 ) *reinterpret_cast<uint4*>( &x[k] ) = *reinterpret_cast<const uint4*>( P + p0 + k );
#pragma unroll
        for ( int k = 0; k < K; ++k ) {
          const int d = int( ( dc[k] >> 16 ) & 0xFFu ), c = int( int16_t( dc[k] & 0xFFFFu ) );
          const int v = int( int16_t( __builtin_bit_cast( uint64_t, x[k] ) >> ( 16 * d ) ) );  // (a shift, not a three-way select: that one became an indexed load from the stack)
          if ( rec[k] != kNoRec && p0 + k >= edge1[k] && v > c ) f2 |= 1u << k;
        }
      }
      {
        uint32_t at = pieceScan<WAVES>( uint32_t( __popc( f2 ) ), sWave[1] );
        uint16_t out[K];
#pragma unroll
        for ( int k = 0; k < K; ++k ) preA[k] = at, out[k] = uint16_t( at ), at += ( f2 >> k ) & 1u;
        preA[K] = at;
        *reinterpret_cast<uint2*>( pre + p0 ) = *reinterpret_cast<const uint2*>( out );
        if ( tid == THREADS - 1 ) pre[kPieceMax] = uint16_t( at );
      }
      pieceBarrier();
      PIECE_MARK( 5)  // second flags + prefix sum
      // ---- per record: the second sweep's edge, the balance rule, the children (records of the next depth, or leaves);
      //      per element: the misplaced right-hand elements of the second sweep ("<= cut" beyond its edge) publish
      const uint32_t base = sNodeBase;
      for ( uint32_t r = tid; r < nc; r += THREADS ) {
        PieceRec*      q  = R + r;
        const uint32_t b = q->begin, e = q->end, e1 = q->edge1, rb2 = pre[e1], re2 = pre[e];
        const uint32_t e2   = e1 + ( ( e - e1 ) - ( re2 - rb2 ) );
        const uint32_t n    = e - b, half = n / 2, lim1 = e1 - b, lim2 = e2 - b;
        const uint32_t idx  = lim1 > half ? lim1 : ( lim2 < half ? lim2 : half );
        const uint32_t mid  = b + idx;
        const uint32_t id0  = base + 2u * r;
        const int      dim  = q->dim;
        const int16_t  cut  = q->cut;
        q->edge2 = uint16_t( e2 ), q->rb2 = uint16_t( rb2 ), q->mid = uint16_t( mid );
        q->lmax = int32_t( 0x80000000 ), q->rmin = 0x7FFFFFFF;
#pragma unroll
        for ( int c = 0; c < 2; ++c ) {
          const uint32_t cb = c ? mid : b, ce = c ? e : mid;
          if ( ce - cb <= uint32_t( kLeafMax ) ) {
            KdNode leaf;
            leaf.a = int32_t( seg.begin + cb ), leaf.b = int32_t( seg.begin + ce ), leaf.divlow = leaf.divhigh = 0, leaf.dim = -1;
            a.nodes[id0 + c] = leaf;
            q->child[c]      = kNoRec;
            deepest          = max( deepest, seg.level + depth + 2u );
          } else {
            const uint32_t slot = atomicAdd( &sCount[cur ^ 1], 1u );
            PieceRec*      ch   = RN + slot;
            ch->begin = uint16_t( cb ), ch->end = uint16_t( ce ), ch->node = id0 + c;
            int16_t l0 = q->lo[0], l1 = q->lo[1], l2 = q->lo[2], h0 = q->hi[0], h1 = q->hi[1], h2 = q->hi[2];
            if ( c == 0 ) {
              if ( dim == 0 ) h0 = cut;
              if ( dim == 1 ) h1 = cut;
              if ( dim == 2 ) h2 = cut;
            } else {
              if ( dim == 0 ) l0 = cut;
              if ( dim == 1 ) l1 = cut;
              if ( dim == 2 ) l2 = cut;
            }
            ch->lo[0] = l0, ch->lo[1] = l1, ch->lo[2] = l2, ch->hi[0] = h0, ch->hi[1] = h1, ch->hi[2] = h2;
            ch->mn[0] = ch->mn[1] = ch->mn[2] = 0x7FFFFFFF, ch->mx[0] = ch->mx[1] = ch->mx[2] = int32_t( 0x80000000 );
            q->child[c] = uint16_t( slot );
          }
        }
      }
      uint32_t edge2[K], rb2[K];
#pragma unroll
      for ( int k = 0; k < K; ++k ) {
        edge2[k] = rb2[k] = 0;
        if ( !waveLive || rec[k] == kNoRec ) continue;
        const uint32_t e = be[k] >> 16, e1 = edge1[k];
        if ( k > 0 && rec[k] == rec[k - 1] ) {
          edge2[k] = edge2[k - 1], rb2[k] = rb2[k - 1];
        } else {
          const uint32_t rb = pre[e1], re = pre[e];
          edge2[k] = e1 + ( ( e - e1 ) - ( re - rb ) ), rb2[k] = rb | ( re << 16 );
        }
        const uint32_t p = p0 + k;
        if ( p >= edge2[k] && !( ( f2 >> k ) & 1u ) ) lst[e1 + ( ( e - p - 1u ) - ( ( rb2[k] >> 16 ) - preA[k + 1] ) )] = uint16_t( p );
      }
      pieceBarrier();
      PIECE_MARK( 6)  // children + second publish
      // (the records of the next depth are counted: their children's node ids, a few passes ahead of their use)
      prevBase = base, prevCount = nc;
      if ( tid == 0 && sCount[cur ^ 1] ) idPending = atomicAdd( a.nodeCount, 2u * sCount[cur ^ 1] );
      // ---- second sweep: the misplaced left-hand elements ("> cut" in [edge1, edge2)) swap
#pragma unroll
      for ( int k = 0; k < K; ++k ) {
        const uint32_t p = p0 + k;
        if ( waveLive && rec[k] != kNoRec && p >= edge1[k] && p < edge2[k] && ( ( f2 >> k ) & 1u ) ) {
          const uint32_t j  = lst[edge1[k] + ( preA[k] - ( rb2[k] & 0xFFFFu ) )];
          const Pt       px = P[p], pj = P[j];
          const uint32_t ip = perm[p], ij = perm[j];
          P[p] = pj, P[j] = px, perm[p] = ij, perm[j] = ip;
        }
      }
      pieceBarrier();
      PIECE_MARK( 7)  // second swaps
      // ---- the elements have landed: tight ranges of the children (one segmented reduction per wavefront where a thread's
      //      positions share a child, LDS atomics where they do not), divlow / divhigh of the parent, record of a position
      if ( waveLive ) {
        uint32_t key[K], mc[K], c1[K];
        bool     same = true;
#pragma unroll
        for ( int k = 0; k < K; ++k ) {
          mc[k] = c1[k] = 0;
          if ( rec[k] != kNoRec ) {
            if ( k > 0 && rec[k] == rec[k - 1] ) {
              mc[k] = mc[k - 1], c1[k] = c1[k - 1];
            } else {
              const PieceHot2 h = *reinterpret_cast<const PieceHot2*>( &R[rec[k]].mid );
              mc[k] = h.midc0, c1[k] = h.c1 & 0xFFFFu;
            }
          }
          key[k] = rec[k] == kNoRec ? kNoKey : 2u * rec[k] + ( p0 + k >= ( mc[k] & 0xFFFFu ) ? 1u : 0u );
          same   = same && key[k] == key[0];
        }
        Pt x[K];
#pragma unroll
        for ( int k = 0; k < K; k += 2 ) *reinterpret_cast<uint4*>( &x[k] ) = *reinterpret_cast<const uint4*>( P + p0 + k );
        uint32_t A = pk2( 0x7FFF, 0x7FFF ), B = pk2( -0x8000, -0x8000 ), C = pk2( 0x7FFF, 0x7FFF );
        if ( same && key[0] != kNoKey ) {
#pragma unroll
          for ( int k = 0; k < K; ++k )
            A = pkMin( A, pk2( x[k].x, x[k].y ) ), B = pkMax( B, pk2( x[k].x, x[k].y ) ), C = pkMin( C, pk2( x[k].z, ~int( x[k].z ) ) );
        }
        const bool head = waveSegMinMaxPacked( same ? key[0] : kNoKey, A, B, C, lane );
        uint16_t out[K];
#pragma unroll
        for ( int k = 0; k < K; ++k ) {
          out[k] = kNoRec;
          if ( key[k] == kNoKey ) continue;
          const uint32_t side = key[k] & 1u;
          const uint32_t cr   = side ? c1[k] : ( mc[k] >> 16 );
          out[k]              = uint16_t( cr );
          if ( same ? ( k > 0 || !head ) : false ) continue;
          int mnx, mny, mnz, mxx, mxy, mxz;
          if ( same )
            mnx = pkLo( A ), mny = pkHi( A ), mnz = pkLo( C ), mxx = pkLo( B ), mxy = pkHi( B ), mxz = ~pkHi( C );
          else
            mnx = mxx = x[k].x, mny = mxy = x[k].y, mnz = mxz = x[k].z;
          PieceRec* q = R + rec[k];
          const int d = int( ( dc[k] >> 16 ) & 0xFFu );
          if ( side == 0 )
            ldsMax( &q->lmax, d == 0 ? mxx : ( d == 1 ? mxy : mxz ) );
          else
            ldsMin( &q->rmin, d == 0 ? mnx : ( d == 1 ? mny : mnz ) );
          if ( cr != kNoRec ) {
            PieceRec* ch = RN + cr;
            ldsMin( &ch->mn[0], mnx ), ldsMin( &ch->mn[1], mny ), ldsMin( &ch->mn[2], mnz );
            ldsMax( &ch->mx[0], mxx ), ldsMax( &ch->mx[1], mxy ), ldsMax( &ch->mx[2], mxz );
          }
        }
        *reinterpret_cast<uint2*>( segOf + p0 ) = *reinterpret_cast<const uint2*>( out );
      }
      cur ^= 1;
    }
    if ( deepest ) atomicMax( &sDepth, deepest );
    if ( PROFILE && threadIdx.x == 0 ) {
      for ( int k = 0; k < 8; ++k ) atomicAdd( a.pieceProfile + k, prof[k] ), prof[k] = 0;
      atomicAdd( a.pieceProfile + 8, 1ull );
    }
    pieceBarrier();
    for ( uint32_t i = tid; i < cnt; i += THREADS ) {
      a.P[seg.begin + i]    = P[i];
      a.perm[seg.begin + i] = perm[i];
    }
    if ( tid == 0 && sDepth ) atomicMax( a.finishDepth, sDepth );
  }
  if ( a.hostDepth && tid == 0 ) {  // the workgroup that is done last hands the deepest level to the host (no copy after the launch)
    __threadfence();
    if ( atomicAdd( a.ticket, 1u ) == gridDim.x - 1u ) {
      __threadfence();
      *a.hostDepth = __hip_atomic_load( a.finishDepth, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
    }
  }
}

}  // namespace

// Builds the tree of d_pts[0..n) on the context's stream into `tree`: points and permutation in tree order, node records
// (root = node 0), root box, depth (levels).  All buffers come from the context's pool.
int buildKdTreeDevice( tmc2_ctx* ctx, const Pt* d_pts, uint64_t n64, DeviceTree& tree ) {
  const uint32_t n = uint32_t( n64 );
  tree.n           = n64;
  tree.depth       = 0;
  for ( int d = 0; d < 3; ++d ) tree.lo[d] = tree.hi[d] = 0;
  if ( n == 0 ) return TMC2_OK;
  hipStream_t    s       = ctx->stream;
  const uint32_t tiles   = ( n + kScanTile - 1 ) / kScanTile;
  const size_t   maxSegs = 2 * ( size_t( n ) / ( kLeafMax + 1 ) + 1 ) + 2;
  const size_t   maxNode = 2 * size_t( n ) + 2;  // (every split takes exactly two ids: hugeSegmentsKernel, pieceKernel, lvDecideKernel)
  TMC2_TRY( tree.ptsTree.alloc( size_t( n ) + 1 ) );  // (one spare Pt: the k-NN kernels load the points in pairs, knn.hip loadLeafPairs)
  TMC2_TRY( tree.perm.alloc( n ) );
  TMC2_TRY( tree.nodes.alloc( maxNode ) );
  DevBuf<uint32_t>   d_work, d_small;
  DevBuf<BuildSeg>   d_segs;
  DevBuf<RetiredSeg> d_retired;
  const size_t       maxRetired = size_t( n ) / ( kLeafMax + 1 ) + 2;  // (retired segments are disjoint and hold > kLeafMax points)
  TMC2_TRY( d_retired.alloc( maxRetired ) );
  DevBuf<HugeSeg> d_huge;
  TMC2_TRY( d_huge.alloc( size_t( n ) / ( kPieceMax + 1 ) + 2 ) );  // (disjoint segments of more than kPieceMax points)
  // Below the level passes: pieces of at most kPieceMax points, one workgroup each, all nodes of a depth at once (pieceKernel);
  // between the two, segments of up to hugeMax points are cut into pieces by one workgroup each (hugeSegmentsKernel: it saves the last
  // few level passes, which move a few dozen segments of 4 097 .. hugeMax points with five chip-wide launches each; option
  // KD_HUGEMAX).  Round 4's three tiers and its level passes (options KD_FORM=tiers, KD_LEVELS=r4 of round 5, kept there as a
  // third cross-check next to the host builder and the oracle) left the library in round 6.
  const auto     hugeEnv = ctxOption( ctx, "KD_HUGEMAX" );
  const uint32_t hugeMax = std::min<uint32_t>( kHugeLimit, std::max<uint32_t>( kPieceMax, hugeEnv ? uint32_t( atoi( hugeEnv->c_str() ) ) : 16384u ) );
  // seg, loc1, loc2, tile totals x 2.  The flag passes read seg and write loc1 / loc2 in groups of 8 positions as 16-byte
  // accesses: each array starts on a 32-byte boundary and is padded to whole groups (what the padding holds is never used).
  const size_t nPad = ( size_t( n ) + 7 ) & ~size_t( 7 );
  TMC2_TRY( d_work.alloc( 3 * nPad + 2 * ( size_t( tiles ) + 1 ) ) );
  TMC2_TRY( d_segs.alloc( 2 * maxSegs ) );
  TMC2_TRY( d_small.alloc( kMaxLevels + 16 ) );  // [0..64] segments per level, then node count, levels, barrier, root box
  static_assert( kMaxLevels + 16 <= 128, "lvRootKernel clears the counters with one workgroup of 128" );
  BuildArgs a;
  a.pts = d_pts, a.n = n, a.tiles = tiles, a.P = tree.ptsTree.p, a.perm = tree.perm.p;
  a.seg = d_work.p, a.loc1 = d_work.p + nPad, a.loc2 = d_work.p + 2 * nPad;
  a.tile1 = d_work.p + 3 * nPad, a.tile2 = a.tile1 + tiles + 1;
  a.segA = d_segs.p, a.segB = d_segs.p + maxSegs, a.nodes = tree.nodes.p;
  a.counts    = d_small.p;
  a.nodeCount = d_small.p + kMaxLevels + 1;
  a.levels    = d_small.p + kMaxLevels + 2;
  a.rootBox   = reinterpret_cast<int32_t*>( d_small.p + kMaxLevels + 8 );
  a.retired      = d_retired.p;
  a.retiredCount = d_small.p + kMaxLevels + 3;
  a.finishDepth  = d_small.p + kMaxLevels + 4;
  a.ticket       = d_small.p + kMaxLevels + 5;
  a.bigCount     = d_small.p + kMaxLevels + 6;
  a.huge         = d_huge.p;
  a.hugeCount    = d_small.p + kMaxLevels + 7;
  a.hugeMax      = hugeMax;
  a.hostSmall    = nullptr;
  a.hostDepth    = ctx->answerLine( tmc2_ctx::kAnswerTreeDepth );
  a.retireMax    = uint32_t( kPieceMax );
  a.splitMax     = uint32_t( kPieceMax );
  // grid-stride launches, two points per lane; the tile kernels take one 2048-point tile per block
  const dim3 blk( kBlock ), grdE( std::max<uint32_t>( 1u, ( n + 2 * kBlock - 1 ) / ( 2 * kBlock ) ) ), grdT( tiles );
  const dim3 grdL( std::max<uint32_t>( 1u, ( n + kLandBlock * kLandRounds - 1 ) / ( kLandBlock * kLandRounds ) ) );
  // the swap passes keep the tile totals in LDS: ( tiles + 1 ) words
  const size_t sumsLds = ( size_t( tiles ) + 1 ) * 4;
  if ( sumsLds > 48 * 1024 ) {
    setError( "kdtree: %u points -- the level passes hold one word per 2 048-point tile in LDS (at most 25 M points)", n );
    return TMC2_E_UNSUPPORTED;
  }
  DevBuf<LvSeg>    d_lv;
  DevBuf<uint16_t> d_list;
  DevBuf<LvPartial> d_partial;
  const size_t     maxLv = 2 * ( size_t( n ) / ( size_t( kPieceMax ) + 1 ) + 2 );  // (segments that split are disjoint and hold > kPieceMax points)
  TMC2_TRY( d_lv.alloc( 2 * maxLv ) );
  TMC2_TRY( d_list.alloc( size_t( tiles ) * kScanTile ) );
  TMC2_TRY( d_partial.alloc( size_t( n ) / ( kLandBlock * kLandRounds ) + 2 ) );
  a.lvA = d_lv.p, a.lvB = d_lv.p + maxLv, a.list = d_list.p, a.partial = d_partial.p;
  const auto decideOpt = ctxOption( ctx, "KD_DECIDE" );  // (test hook: "global" = the fold of a level of more than kDecideRng segments)
  a.decideRng = decideOpt && ( *decideOpt )[0] == 'g' ? 0u : uint32_t( kDecideRng );
  hipLaunchKernelGGL( lvRootKernel, dim3( 1 ), dim3( 128 ), 0, s, a );
  hipLaunchKernelGGL( lvInitKernel, dim3( std::min<uint32_t>( grdE.x, 1024u ) ), blk, 0, s, a );  // (each workgroup reports the root's range once)
  hipLaunchKernelGGL( lvDecideKernel, dim3( 1 ), dim3( kDecideThreads ), 0, s, a, 0u );
  uint32_t out[kMaxLevels + 16];
  int      found = -1;
  // How many levels the passes run is only known on the device.  Frames of a sequence are alike: the count of the last tree
  // of about this size (kept in the context) is queued back to back and then checked; without it, the levels that cannot be
  // the last; afterwards two at a time per read-back (launches past the last level find nothing to do).
  int& hint = ctx->kdLevelHint[( n >> 15 ) * 2u + 1u];
  for ( uint32_t level = 0; level < uint32_t( kMaxLevels ) && found < 0; ) {
    uint32_t chunkEnd = level + 1;
    if ( level == 0 && hint > 0 ) {
      chunkEnd = uint32_t( std::min( hint, kMaxLevels ) );
    } else {
      while ( chunkEnd < uint32_t( kMaxLevels ) && ( uint64_t( hugeMax ) << std::min<uint32_t>( chunkEnd - 1, 40 ) ) < n ) ++chunkEnd;
      if ( chunkEnd == level + 1 ) chunkEnd = std::min<uint32_t>( level + 2, kMaxLevels );
    }
    volatile uint32_t* hostSmall = ctx->answerLine( tmc2_ctx::kAnswerTreeLevels );  // (kMaxLevels + 16 = 80 words: five lines)
    for ( ; level < chunkEnd; ++level ) {
      hipLaunchKernelGGL( lvFlagKernel<true>, grdT, blk, 0, s, a, level );
      hipLaunchKernelGGL( lvSwapOneKernel, grdE, blk, sumsLds, s, a, level );
      hipLaunchKernelGGL( lvFlagKernel<false>, grdT, blk, 0, s, a, level );
      hipLaunchKernelGGL( lvSwapTwoKernel, grdL, dim3( kLandBlock ), sumsLds, s, a, level );
      BuildArgs ad = a;
      if ( level + 1 == chunkEnd ) ad.hostSmall = hostSmall;  // (the batch's last decide pass publishes the counters: no copy)
      hipLaunchKernelGGL( lvDecideKernel, dim3( 1 ), dim3( kDecideThreads ), 0, s, ad, level + 1u );
    }
    TMC2_HIP( hipGetLastError() );
    TMC2_HIP( hipStreamSynchronize( s ) );
    for ( int w = 0; w < kMaxLevels + 16; ++w ) out[w] = hostSmall[w];
    for ( uint32_t l = 0; l <= level && l <= uint32_t( kMaxLevels ); ++l )
      if ( out[l] == 0 ) {
        found = int( l );
        break;
      }
  }
  if ( found < 0 ) {
    setError( "kdtree: more than %d levels", kMaxLevels - 1 );
    return TMC2_E_UNSUPPORTED;
  }
  tree.depth = found;
  hint       = std::max( found, 1 );
  const int32_t* box = reinterpret_cast<const int32_t*>( out + kMaxLevels + 8 );
  for ( int d = 0; d < 3; ++d ) tree.lo[d] = box[d], tree.hi[d] = box[3 + d];
  // everything below the level passes: one workgroup per piece
  const uint32_t hugeSegs = out[kMaxLevels + 7];
  if ( hugeSegs )  // (segments of up to hugeMax points: one workgroup each cuts its segment into pieces, which join the list)
    hipLaunchKernelGGL( hugeSegmentsKernel, dim3( std::min<uint32_t>( hugeSegs, 4u * uint32_t( ctx->cuCount ) ) ), dim3( 64 * kHugeWaves ), 0, s, a );
  const uint32_t retired = out[kMaxLevels + 3] + hugeSegs * ( 2u * hugeMax / uint32_t( kPieceMax ) );
  if ( retired ) {
    const dim3 grid( std::min<uint32_t>( retired, 8u * uint32_t( ctx->cuCount ) ) ), block( kPieceMax / kPiecePer );
    if ( ctxOption( ctx, "KD_PIECE_PROFILE" ) ) {  // diagnostic: where a depth's time goes (thread 0 of every workgroup, between barriers)
      DevBuf<unsigned long long> d_prof;
      TMC2_TRY( d_prof.alloc( 16 ) );
      TMC2_HIP( hipMemsetAsync( d_prof.p, 0, 16 * 8, s ) );
      a.pieceProfile = d_prof.p;
      TMC2_TRY( allowLargeLds( reinterpret_cast<const void*>( pieceKernel<true> ), kPieceLdsBytes, ctx->device, 256 ) );
      hipLaunchKernelGGL( pieceKernel<true>, grid, block, kPieceLdsBytes, s, a );
      unsigned long long h[16];
      TMC2_HIP( hipMemcpyAsync( h, d_prof.p, sizeof( h ), hipMemcpyDeviceToHost, s ) );
      TMC2_HIP( hipStreamSynchronize( s ) );
      static const char* what[8] = {"landing of the previous depth", "node records + split rules", "first flags + prefix sum", "first publish",
                                    "first swaps", "second flags + prefix sum", "children + second publish", "second swaps"};
      fprintf( stderr, "pieceKernel: %llu pieces, us per piece between the barriers of its depths (thread 0 of each workgroup):", h[8] );
      for ( int k = 0; k < 8; ++k ) fprintf( stderr, " %s %.1f |", what[k], 0.01 * double( h[k] ) / double( std::max<unsigned long long>( h[8], 1 ) ) );
      fprintf( stderr, "\n" );
    } else {
      TMC2_TRY( allowLargeLds( reinterpret_cast<const void*>( pieceKernel<> ), kPieceLdsBytes, ctx->device, 256 ) );
      hipLaunchKernelGGL( pieceKernel<>, grid, block, kPieceLdsBytes, s, a );
    }
    TMC2_HIP( hipGetLastError() );
    TMC2_HIP( hipStreamSynchronize( s ) );
    const uint32_t fin = *a.hostDepth;
    if ( fin >= uint32_t( kMaxLevels ) ) {
      setError( "kdtree: more than %d levels", kMaxLevels - 1 );
      return TMC2_E_UNSUPPORTED;
    }
    tree.depth = std::max( tree.depth, int( fin ) );
  }
  return TMC2_OK;
}

}  // namespace tmc2
