// union_find.h -- the lock-free union-find of S7 (connected components, patches.hip) and S3 (contraction of the orientation
// graph, orient_contract.hip).  Device-only.
//
// One 32-bit link word per element.  UnionFind<false>: the word is the parent.  UnionFind<true>: the word is
// parent << 1 | parity-to-parent (S3: 1 = the normals of the element and of its parent get opposite signs).  A root links to
// itself (parity 0).  Why concurrent finds and unions, reading views that lag behind each other, still end in the right forest:
//   * Links only ever FALL in hashed priority (ufPriority; hooking by index would grow chains as long as the scan order of the
//     cloud).  The initial forests of the two users obey that, a hook puts the root of larger priority under the other, and path
//     halving replaces a link by the grandparent's.  So the forest is acyclic at every moment and in every view, and every
//     climb ends.
//   * Every word ever stored states a true relation: it names a member of the same set (sets only grow) and, with PARITY, the
//     parity it carries is the composition of true parities.  A STALE read -- the climbs read through the XCD's L2
//     (loadStaleOk: workgroup scope, the view of this XCD, possibly behind the other seven) -- therefore yields an ancestor-or-
//     self of the truth with its right parity: it costs a detour, never a wrong answer.  An agent-scope load per hop would be
//     a trip past the L2 for every link of every path.
//   * Only the confirming step, "is this really a root", runs at agent scope (the coherent level) and climbs on from there if it
//     is not; the hook is a compare-and-swap on the root's own word, which fails if anyone hooked or was hooked there first.
//   * true from the store-free pre-check (sameSetStale) is final for the same reason: the two climbs met at a common ancestor
//     through words that each link two members of one set.  false only means "not known in this view".
//   * The flat view ("root of every element", read by later kernels as flat) goes to an array of its OWN, never back into the
//     link words: a path-halving store issued from a stale view by a find that passes through x at the same moment could land
//     after the flat root and leave word[x] short of it.  Rare while the union pass compresses nearly every path, frequent once
//     most edges end in the store-free pre-check.
#pragma once
#include "internal.h"

#if defined( __HIPCC__ )
namespace tmc2 {

__device__ __forceinline__ uint32_t ufPriority( uint32_t x ) { return x * 2654435761u; }  // odd multiplier: a bijection

constexpr uint32_t kUfBroken = 0xFFFFFFFFu;  // rootCoherent: a link that does not fall in priority, or leaves [0, n)

struct UfRoot {
  uint32_t root, parity;  // parity of the element relative to the root (plain: 0)
};

template <bool PARITY>
struct UnionFind {
  static __device__ __forceinline__ uint32_t parentOf( uint32_t w ) {
    if constexpr ( PARITY )
      return w >> 1;
    else
      return w;
  }
  static __device__ __forceinline__ uint32_t link( uint32_t parent, uint32_t parity ) {
    if constexpr ( PARITY )
      return ( parent << 1 ) | parity;
    else
      return parent;
  }

  // Root of x (and the parity of x relative to it); halves the path on the way: one stale load per hop, the parent's word is
  // carried forward; halved links are stored at agent scope; then the coherent confirmation.
  static __device__ __forceinline__ UfRoot find( uint32_t* word, uint32_t x, bool agent ) {
    uint32_t acc = 0;
    uint32_t w   = loadStaleOk( &word[x], agent );
    while ( parentOf( w ) != x ) {
      const uint32_t p = parentOf( w ), wp = loadStaleOk( &word[p], agent );
      if ( parentOf( wp ) != p )  // (parity of the halved link: x -> p composed with p -> its parent)
        __hip_atomic_store( &word[x], link( parentOf( wp ), ( w ^ wp ) & 1u ), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
      if constexpr ( PARITY ) acc ^= w & 1u;
      x = p;
      w = wp;
    }
    for ( ;; ) {
      w = __hip_atomic_load( &word[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
      if ( parentOf( w ) == x ) return {x, acc};
      if constexpr ( PARITY ) acc ^= w & 1u;
      x = parentOf( w );
    }
  }

  // "Are a and b in one set already?" from this CU's possibly stale view, without a store or an atomic.  The end of LARGER
  // priority climbs (priorities fall along every link, so the end of smaller priority cannot lie below the other one's path);
  // the two meet at a common ancestor if the view has one.  Whether the parities along the two paths agree with an edge is not
  // this walk's business.  Most edges join elements that the initial forest or an earlier union has put into one tree already:
  // they end here, a few L1 / L2 hits each.
  static __device__ __forceinline__ bool sameSetStale( const uint32_t* word, uint32_t a, uint32_t b, bool agent ) {
    uint32_t pa = ufPriority( a ), pb = ufPriority( b );
    for ( ;; ) {
      if ( a == b ) return true;
      if ( pa < pb ) {
        const uint32_t t = a;
        a                = b;
        b                = t;
        const uint32_t q = pa;
        pa               = pb;
        pb               = q;
      }
      const uint32_t up = parentOf( loadStaleOk( &word[a], agent ) );
      if ( up == a ) return false;  // a root of larger priority than b: nothing above it in this view
      a  = up;
      pa = ufPriority( a );
    }
  }

  // Joins the sets of a and b; s (PARITY): the parity of a relative to b that the joining edge demands.  Whether an edge whose
  // ends are in one set already agrees with the parities there is for the caller to check on the settled forest.
  static __device__ __forceinline__ void unite( uint32_t* word, uint32_t a, uint32_t b, uint32_t s, bool agent ) {
    for ( ;; ) {
      const UfRoot ra = find( word, a, agent ), rb = find( word, b, agent );
      a = ra.root, b = rb.root;
      if ( a == b ) return;
      if constexpr ( PARITY ) s ^= ra.parity ^ rb.parity;  // now the parity of root a relative to root b (symmetric)
      if ( ufPriority( a ) < ufPriority( b ) ) {
        const uint32_t t = a;
        a                = b;
        b                = t;
      }
      // hook the root of larger priority under the other; a failed attempt goes on from the two (former) roots
      if ( atomicCAS( &word[a], link( a, 0u ), link( b, s ) ) == link( a, 0u ) ) return;
    }
  }

  // Debug invariants (UF_CHECK): the root of x on the settled forest, by a bounded climb at agent scope only (the coherent
  // truth, no stale view involved); kUfBroken on a link that does not fall in priority or that leaves [0, n).
  static __device__ __forceinline__ uint32_t rootCoherent( const uint32_t* word, uint32_t x, uint32_t n ) {
    for ( uint32_t hops = 0; hops <= n; ++hops ) {
      const uint32_t q = parentOf( __hip_atomic_load( &word[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ) );
      if ( q == x ) return x;
      if ( q >= n || ufPriority( q ) >= ufPriority( x ) ) return kUfBroken;
      x = q;
    }
    return kUfBroken;
  }
};

}  // namespace tmc2
#endif
