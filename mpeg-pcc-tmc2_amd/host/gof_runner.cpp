// gof_runner.cpp -- libtmc2gof.so: the frame loop of a GOF pass as native host code over the C-ABI of libtmc2hip.so
// (include/tmc2gof.h).  No device code and no HIP call here: threads, the call sequence of INTEGRATION.md section 4, one rendezvous.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include "tmc2gof.h"

namespace {
// the message of the LAST call of the calling thread (two GOFs encoded from two threads do not overwrite each other's; a pass
// collects the message of whichever of its slot threads failed first and hands it to its caller's thread on return)
thread_local std::string t_err;

// One core per slot, round-robin over the last-level caches (SMT siblings dropped); empty if the topology cannot be read.
// The mask is the PROCESS' (its main thread's), not the calling thread's: a caller that has pinned itself to one core (a worker of
// another pool) must not pin every slot thread of every later pass to that core.  Reading the topology costs milliseconds, so the
// list is kept per mask.
std::vector<int> coresOf( const cpu_set_t& allowed );
std::vector<int> coresByCacheDomain() {
  cpu_set_t allowed;
  CPU_ZERO( &allowed );
  if ( sched_getaffinity( getpid(), sizeof( allowed ), &allowed ) != 0 ) return {};
  static std::mutex       lock;
  static cpu_set_t        cachedMask;
  static std::vector<int> cached;
  static bool             have = false;
  std::lock_guard<std::mutex> g( lock );
  if ( !have || !CPU_EQUAL( &allowed, &cachedMask ) ) cached = coresOf( allowed ), cachedMask = allowed, have = true;
  return cached;
}
std::vector<int> coresOf( const cpu_set_t& allowed ) {
  std::map<std::string, std::vector<int>> domains;
  for ( int cpu = 0; cpu < CPU_SETSIZE; ++cpu ) {
    if ( !CPU_ISSET( cpu, &allowed ) ) continue;
    const std::string base = "/sys/devices/system/cpu/cpu" + std::to_string( cpu ) + "/";
    std::ifstream     sib( base + "topology/thread_siblings_list" ), l3( base + "cache/index3/shared_cpu_list" );
    std::string       s, d;
    if ( !std::getline( sib, s ) || !std::getline( l3, d ) ) return {};
    if ( std::atoi( s.c_str() ) != cpu ) continue;
    domains[d].push_back( cpu );
  }
  std::vector<int> order;
  for ( size_t k = 0;; ++k ) {
    bool any = false;
    for ( auto& kv : domains )
      if ( k < kv.second.size() ) order.push_back( kv.second[k] ), any = true;
    if ( !any ) break;
  }
  return order;
}
int coreOfSlot( const std::vector<int>& cores, int slot ) { return cores.empty() || slot < 0 ? -1 : cores[size_t( slot ) % cores.size()]; }

// the CTC lossy settings (cfg/common/ctc-common.cfg + the sequence's), as tmc2_amd.lib.ctc_params
tmc2_segmenter_params ctcParams( const tmc2_gof_config& c, const double w[3] ) {
  tmc2_segmenter_params p{};
  p.nnNormalEstimation = 16, p.normalOrientation = 1, p.gridBasedRefineSegmentation = 1, p.maxNNCountRefineSegmentation = 1024;
  p.iterationCountRefineSegmentation = c.iterationCountRefineSegmentation;
  p.voxelDimensionRefineSegmentation = c.voxelDimensionRefineSegmentation, p.searchRadiusRefineSegmentation = 192;
  p.occupancyResolution = 16, p.enablePatchSplitting = 1, p.maxPatchSize = 1024, p.quantizerSizeX = 16, p.quantizerSizeY = 16;
  p.minPointCountPerCCPatchSegmentation = 16, p.maxNNCountPatchSegmentation = 16, p.surfaceThickness = 4, p.mapCountMinus1 = 1;
  p.minLevel = 64, p.maxAllowedDepth = 255, p.geometryBitDepth2D = 8, p.geometryBitDepth3D = c.geometryBitDepth3D;
  p.maxAllowedDist2RawPointsDetection = 9, p.maxAllowedDist2RawPointsSelection = 1, p.lambdaRefineSegmentation = 3;
  for ( int k = 0; k < 3; ++k ) p.weightNormal[k] = w[k];
  return p;
}

// What a pass knows of its own failure: the first failing status and the message that goes with it, from whichever thread.
struct Pass {
  std::atomic<int> status{TMC2_OK};
  std::mutex       lock;
  std::string      message;
  bool             failed() const { return status.load() != TMC2_OK; }
  void             fail( int rc, const std::string& why ) {
    int expected = TMC2_OK;
    if ( status.compare_exchange_strong( expected, rc ) ) {
      std::lock_guard<std::mutex> g( lock );
      message = why;
    }
  }
  void failCall( int rc, const char* call ) { fail( rc, std::string( call ) + ": " + tmc2_last_error() ); }  // (the failing thread's own message)
  // an exception a slot thread caught: the status always, the text if there is memory for it
  void caught( const char* what ) noexcept {
    try {
      fail( TMC2_E_STATE, std::string( "slot thread: " ) + what );
    } catch ( const std::exception& ) {
      int expected = TMC2_OK;
      status.compare_exchange_strong( expected, TMC2_E_STATE );
    }
  }
  int done() {  // on the calling thread: the pass' status, its message for tmc2_gof_last_error()
    std::lock_guard<std::mutex> g( lock );
    t_err = message;
    return status.load();
  }
};
#define GOF_TRY( call )                               \
  do {                                                \
    const int rc_ = ( call );                         \
    if ( rc_ != TMC2_OK ) {                           \
      s.pass.failCall( rc_, #call );                  \
      return;                                         \
    }                                                 \
  } while ( 0 )

// The slot threads of the passes: parked between passes instead of being born and joined twice per pass (32 births per 180 ms GOF
// with sixteen slots).  A pass LEASES as many as it has slots -- two passes of two caller threads never share a thread -- and hands
// them back when its phase is over; the set only grows.  Never destroyed (a thread parked in a condition variable whose owner's
// destructor runs at exit is the classic way to hang a process on its way out).
class SlotThreads {
  struct Worker {
    std::mutex              lock;
    std::condition_variable wake;
    std::function<void()>   job;
    int                     pinned = -1;
    std::thread             thread;
  };
  std::mutex                           lock_;
  std::vector<std::unique_ptr<Worker>> all_;
  std::vector<Worker*>                 idle_;
  static void loop( Worker* w ) {
    for ( ;; ) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> g( w->lock );
        w->wake.wait( g, [&] { return bool( w->job ); } );
        job.swap( w->job );
      }
      job();
    }
  }

 public:
  static SlotThreads& instance() {
    static SlotThreads* pool = new SlotThreads();  // (leaked on purpose: see above)
    return *pool;
  }
  // fn( slot ) on `slots` threads side by side, slot s pinned to cores[s % cores.size()]; returns when all are done.  Nothing may
  // unwind a parked thread: what fn throws fails the pass (Pass::caught) before the slot signals that it is done.
  void run( int slots, const std::vector<int>& cores, Pass& pass, const std::function<void( int )>& fn ) {
    std::vector<Worker*> mine;
    {
      std::lock_guard<std::mutex> g( lock_ );
      while ( int( mine.size() ) < slots ) {
        if ( idle_.empty() ) {
          all_.emplace_back( new Worker() );
          Worker* w = all_.back().get();
          w->thread = std::thread( loop, w );
          w->thread.detach();
          idle_.push_back( w );
        }
        mine.push_back( idle_.back() );
        idle_.pop_back();
      }
    }
    std::mutex              doneLock;
    std::condition_variable doneCv;
    int                     left = slots;
    for ( int sl = 0; sl < slots; ++sl ) {
      Worker*   w    = mine[size_t( sl )];
      const int core = coreOfSlot( cores, sl );
      std::lock_guard<std::mutex> g( w->lock );
      w->job = [&, w, sl, core] {
        if ( core >= 0 && w->pinned != core ) {
          cpu_set_t one;
          CPU_ZERO( &one );
          CPU_SET( core, &one );
          (void)pthread_setaffinity_np( pthread_self(), sizeof( one ), &one );
          w->pinned = core;
        }
        try {
          fn( sl );
        } catch ( const std::exception& e ) {
          pass.caught( e.what() );
        } catch ( ... ) {
          pass.caught( "unknown exception" );
        }
        std::lock_guard<std::mutex> d( doneLock );
        if ( --left == 0 ) doneCv.notify_one();
      };
      w->wake.notify_one();
    }
    {
      std::unique_lock<std::mutex> d( doneLock );
      doneCv.wait( d, [&] { return left == 0; } );
    }
    std::lock_guard<std::mutex> g( lock_ );
    for ( Worker* w : mine ) idle_.push_back( w );
  }
};
}  // namespace

extern "C" const char* tmc2_gof_last_error( void ) { return t_err.c_str(); }
extern "C" int         tmc2_gof_slot_core( int slot ) { return coreOfSlot( coresByCacheDomain(), slot ); }


// ---- the ranks of a sharded GOF (one process per GPU): RCCL, loaded at run time --------------------------------------------
// (librccl.so is looked up when a communicator is made, not when this library is loaded: a single-GPU host needs no RCCL.  The
//  test tier loads a recorder in its place through TMC2_RCCL_LIBRARY, tests/mock/mock_rccl.cpp.)
namespace {
struct NcclId {
  char internal[128];
};
enum { kNcclUint8 = 1, kNcclInt32 = 2, kNcclFloat64 = 8, kNcclMax = 2 };
struct Rccl {
  void* lib = nullptr;
  int ( *GetUniqueId )( NcclId* )                                                         = nullptr;
  int ( *CommInitRank )( void**, int, NcclId, int )                                       = nullptr;
  int ( *CommDestroy )( void* )                                                           = nullptr;
  int ( *CommAbort )( void* )                                                             = nullptr;  // (optional)
  int ( *Broadcast )( const void*, void*, size_t, int, int, void*, void* )                = nullptr;
  int ( *AllReduce )( const void*, void*, size_t, int, int, void*, void* )                = nullptr;
  int ( *Send )( const void*, size_t, int, int, void*, void* )                            = nullptr;
  int ( *Recv )( void*, size_t, int, int, void*, void* )                                  = nullptr;
  int ( *GroupStart )()                                                                   = nullptr;
  int ( *GroupEnd )()                                                                     = nullptr;
  const char* ( *GetErrorString )( int )                                                  = nullptr;
  bool load( std::string& why ) {
    const char* named = getenv( "TMC2_RCCL_LIBRARY" );
    for ( const char* name : {named, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"} ) {
      if ( !name ) continue;
      lib = dlopen( name, RTLD_NOW | RTLD_LOCAL );
      if ( lib ) break;
      why = dlerror();
    }
    if ( !lib ) return false;
    const auto sym = [&]( const char* n, bool required = true ) {
      void* p = dlsym( lib, n );
      if ( !p && required ) why = std::string( "librccl: no symbol " ) + n;
      return p;
    };
    GetUniqueId    = reinterpret_cast<decltype( GetUniqueId )>( sym( "ncclGetUniqueId" ) );
    CommInitRank   = reinterpret_cast<decltype( CommInitRank )>( sym( "ncclCommInitRank" ) );
    CommDestroy    = reinterpret_cast<decltype( CommDestroy )>( sym( "ncclCommDestroy" ) );
    CommAbort      = reinterpret_cast<decltype( CommAbort )>( sym( "ncclCommAbort", false ) );
    Broadcast      = reinterpret_cast<decltype( Broadcast )>( sym( "ncclBroadcast" ) );
    AllReduce      = reinterpret_cast<decltype( AllReduce )>( sym( "ncclAllReduce" ) );
    Send           = reinterpret_cast<decltype( Send )>( sym( "ncclSend" ) );
    Recv           = reinterpret_cast<decltype( Recv )>( sym( "ncclRecv" ) );
    GroupStart     = reinterpret_cast<decltype( GroupStart )>( sym( "ncclGroupStart" ) );
    GroupEnd       = reinterpret_cast<decltype( GroupEnd )>( sym( "ncclGroupEnd" ) );
    GetErrorString = reinterpret_cast<decltype( GetErrorString )>( sym( "ncclGetErrorString" ) );
    return GetUniqueId && CommInitRank && CommDestroy && Broadcast && AllReduce && Send && Recv && GroupStart && GroupEnd && GetErrorString;
  }
};
}  // namespace

struct tmc2_gof_comm {
  int       rank = 0, world = 1;
  tmc2_ctx* ctx  = nullptr;  // a context on this rank's device: its stream carries the collectives
  Rccl      rccl;
  void*     comm    = nullptr;
  void*     dSmall  = nullptr;  // 64 bytes on the device: weights, heights, headers
  void*     dBlocks = nullptr;  // the records of this rank's frames, then (rank 0) those of every rank
  size_t    blocksBytes = 0;
  int64_t   passes  = 0;        // passes this communicator has carried (the ranks call them in lock-step: every block carries it)
  bool      broken  = false;    // a collective failed or timed out: the communicator was aborted, every later call is refused
  std::mutex abortLock;         // (the watchdog's thread and the calling thread both may abort: once)
  double    timeoutSeconds = 600.0;
  std::vector<uint8_t> hostBlocks;
};

namespace {
void breakComm( tmc2_gof_comm* comm ) {  // a collective failed: nobody may be left waiting for this rank's part of it, no later call may use it
  std::lock_guard<std::mutex> g( comm->abortLock );
  if ( comm->comm && comm->rccl.CommAbort ) (void)comm->rccl.CommAbort( comm->comm ), comm->comm = nullptr;
  comm->broken = true;
}
// A rank that waits in a collective for a rank that will never arrive (it died, or left the pass through a path that skipped the
// collective) would wait for ever -- in the call itself (a group's connection set-up) or in the stream synchronisation behind it.
// Every collective of this file therefore runs under a watchdog: when it is not over after comm->timeoutSeconds
// (TMC2_GOF_COLLECTIVE_TIMEOUT, default 600 s: far beyond any pass) the communicator is ABORTED from the watchdog's thread
// (ncclCommAbort: pending calls and kernels give up, the synchronisation returns) and the call fails with TMC2_E_STATE.
class Watchdog {
  tmc2_gof_comm*          comm_;
  std::mutex              lock_;
  std::condition_variable cv_;
  bool                    done_ = false, fired_ = false;
  std::thread             thread_;

 public:
  explicit Watchdog( tmc2_gof_comm* comm ) : comm_( comm ) {
    if ( !comm_->rccl.CommAbort || comm_->timeoutSeconds <= 0.0 ) return;
    thread_ = std::thread( [this] {
      std::unique_lock<std::mutex> g( lock_ );
      if ( cv_.wait_for( g, std::chrono::duration<double>( comm_->timeoutSeconds ), [this] { return done_; } ) ) return;
      fired_ = true;
      g.unlock();
      breakComm( comm_ );
    } );
  }
  bool finish() {  // -> true if the watchdog had to abort the communicator
    if ( thread_.joinable() ) {
      {
        std::lock_guard<std::mutex> g( lock_ );
        done_ = true;
      }
      cv_.notify_one();
      thread_.join();
    }
    return fired_;
  }
  ~Watchdog() { (void)finish(); }
};
#define HIP_TRY( call, what )                              \
  do {                                                     \
    const int rc_ = ( call );                              \
    if ( rc_ != TMC2_OK ) {                                \
      t_err = std::string( what ) + ": " + tmc2_last_error(); \
      return rc_;                                          \
    }                                                      \
  } while ( 0 )
int ncclFailed( tmc2_gof_comm* comm, int rc, const char* what ) {  // a failed RCCL call: its text, the communicator aborted
  t_err = std::string( what ) + ": " + ( comm->rccl.GetErrorString ? comm->rccl.GetErrorString( rc ) : "?" );
  breakComm( comm );
  return TMC2_E_HIP;
}
int refuseBroken( tmc2_gof_comm* comm ) {
  if ( !comm->broken ) return TMC2_OK;
  t_err = "tmc2_gof_comm: the communicator was aborted after a collective failed or timed out; make a new one";
  return TMC2_E_STATE;
}

// ncclGroupStart .. ncclGroupEnd around the calls handed to then(): once the group is open it is ALWAYS closed (an open group is the
// thread's, and would swallow the calls of the next communicator made on it); the first error inside is the group's, and no call
// is enqueued after it.
class Group {
  const Rccl& rccl_;
  int         first_;
  bool        open_;

 public:
  explicit Group( const Rccl& rccl ) : rccl_( rccl ), first_( rccl.GroupStart() ), open_( first_ == 0 ) {}
  template <typename Call>
  void then( Call&& call ) {
    if ( first_ == 0 ) first_ = call();
  }
  int end() {  // -> the first error of the group, 0 if none
    if ( open_ ) {
      open_        = false;
      const int rc = rccl_.GroupEnd();
      if ( first_ == 0 ) first_ = rc;
    }
    return first_;
  }
  ~Group() { (void)end(); }
};

// ONE collective, the whole dance: a broken communicator is refused; under the watchdog the words to send go up, the collective is
// issued, and the wait behind it is a download of the answer or (nothing to bring back) a synchronisation.  Every rank ALWAYS
// issues the collective -- one whose upload failed still takes part, with whatever the buffer holds, and reports its own failure
// LAST, so that nobody waits for it; the stage behind the collective carries the failure.  issue( stream ) -> RCCL's status.
struct Copy {
  void*  host   = nullptr;
  void*  device = nullptr;
  size_t bytes  = 0;  // 0: no copy
};
template <typename Issue>
int collective( tmc2_gof_comm* comm, const char* what, Copy up, Issue&& issue, Copy down ) {
  if ( const int rc = refuseBroken( comm ) ) return rc;
  Watchdog    dog( comm );
  std::string upError;
  const int   upRc = up.bytes ? tmc2_ctx_upload( comm->ctx, up.device, up.host, up.bytes ) : TMC2_OK;
  if ( upRc != TMC2_OK ) upError = std::string( what ) + ": upload: " + tmc2_last_error();
  int rc = TMC2_OK;
  if ( const int nccl = issue( tmc2_ctx_stream( comm->ctx ) ) ) {
    rc = ncclFailed( comm, nccl, what );
  } else {
    rc = down.bytes ? tmc2_ctx_download( comm->ctx, down.host, down.device, down.bytes ) : tmc2_ctx_synchronize( comm->ctx );
    if ( rc != TMC2_OK ) t_err = std::string( what ) + ": " + tmc2_last_error();
    if ( upRc != TMC2_OK ) t_err = upError, rc = upRc;
  }
  if ( dog.finish() ) {
    t_err = std::string( what ) + ": no answer from the other ranks within " + std::to_string( int( comm->timeoutSeconds ) ) +
            " s (TMC2_GOF_COLLECTIVE_TIMEOUT): the communicator was aborted";
    return TMC2_E_STATE;
  }
  return rc;
}
// `count` words of `width` bytes from rank 0 to everybody (the axis weights of frame 0: PCCEncoder::calculateWeightNormal runs on
// the first frame only; the canvas of a chained GOF)
int commBroadcast( tmc2_gof_comm* comm, void* host, size_t count, int type, size_t width, const char* what ) {
  const Copy words{host, comm->dSmall, count * width};
  return collective( comm, what, words, [&]( void* st ) { return comm->rccl.Broadcast( comm->dSmall, comm->dSmall, count, type, 0, comm->comm, st ); }, words );
}
// max over the ranks of `count` int32 words (count <= 16): the canvas height of the GOF is the max of what the ranks' frames packed
// into (resizeGeometryVideo, PCCEncoder.cpp:5546-5591)
int commMax( tmc2_gof_comm* comm, int32_t* host, size_t count, const char* what ) {
  const Copy words{host, comm->dSmall, 4 * count};
  return collective( comm, what, words, [&]( void* st ) { return comm->rccl.AllReduce( comm->dSmall, comm->dSmall, count, kNcclInt32, kNcclMax, comm->comm, st ); }, words );
}
// every rank's block of `mine` bytes (hostBlocks[0 .. mine)) to rank 0 (hostBlocks[mine * (r + 1) ..)): one grouped send / receive
// (an upload that failed lets a stale block travel; its pass number gives it away)
int commBlocksToRoot( tmc2_gof_comm* comm, size_t mine, const char* what ) {
  uint8_t*   host = comm->hostBlocks.data();
  uint8_t*   dev  = static_cast<uint8_t*>( comm->dBlocks );
  const bool root = comm->rank == 0;
  const auto exchange = [&]( void* st ) {
    Group group( comm->rccl );
    for ( int r = 0; root && r < comm->world; ++r )
      group.then( [&] { return comm->rccl.Recv( dev + mine * size_t( r + 1 ), mine, kNcclUint8, r, comm->comm, st ); } );
    group.then( [&] { return comm->rccl.Send( dev, mine, kNcclUint8, 0, comm->comm, st ); } );
    return group.end();
  };
  return collective( comm, what, {host, dev, mine}, exchange, root ? Copy{host + mine, dev + mine, mine * size_t( comm->world )} : Copy{} );
}
// rank 0's block for rank r (hostBlocks[mine * r ..), r = 0 .. world-1) to rank r (hostBlocks[0 .. mine)): the way back
int commBlocksFromRoot( tmc2_gof_comm* comm, size_t mine, const char* what ) {
  uint8_t*   host = comm->hostBlocks.data();
  uint8_t*   dev  = static_cast<uint8_t*>( comm->dBlocks );
  const bool root = comm->rank == 0;
  const auto exchange = [&]( void* st ) {
    Group group( comm->rccl );
    for ( int r = 0; root && r < comm->world; ++r )
      group.then( [&] { return comm->rccl.Send( dev + mine * size_t( r + 1 ), mine, kNcclUint8, r, comm->comm, st ); } );
    group.then( [&] { return comm->rccl.Recv( dev, mine, kNcclUint8, 0, comm->comm, st ); } );
    return group.end();
  };
  return collective( comm, what, root ? Copy{host, dev + mine, mine * size_t( comm->world )} : Copy{}, exchange, {host, dev, mine} );
}

int ensureBlocks( tmc2_gof_comm* comm, size_t need ) {
  if ( need <= comm->blocksBytes ) return TMC2_OK;
  if ( comm->dBlocks ) HIP_TRY( tmc2_ctx_device_free( comm->ctx, comm->dBlocks ), "records: free" );
  comm->dBlocks = nullptr, comm->blocksBytes = 0;
  HIP_TRY( tmc2_ctx_device_alloc( comm->ctx, need, &comm->dBlocks ), "records: device buffer" );
  comm->blocksBytes = need;
  return TMC2_OK;
}

constexpr size_t roundUp( size_t n, size_t to ) { return ( n + to - 1 ) / to * to; }

// One frame's block on the wire: a header of int64 words, `slots` records, with the packed lists one int32 per record slot (the
// patch each was matched to), a pool of block occupancy.  Three blocks travel, told apart by the header word that carries the
// pass number (a block of another pass, or of impossible sizes, is not read):
//   the final gather     [count, PASS]                                 records
//   records to rank 0    [count, pool bytes, PASS, 0]                  records, pool
//   packed lists back    [count, pool bytes, tile (W << 32 | H), PASS] records, matches, pool
struct Block {
  enum Kind { kGather = 1, kToRoot = 2, kFromRoot = 3 };  // (= the header word of the pass number)
  Kind   kind;
  size_t slots, pool;  // record slots; pool bytes, a multiple of 64
  size_t recordsAt() const { return kind == kGather ? 16 : 32; }
  size_t matchesAt() const { return recordsAt() + slots * sizeof( tmc2_patch ); }
  size_t poolAt() const { return matchesAt() + ( kind == kFromRoot ? 4 * slots : 0 ); }
  size_t bytes() const { return poolAt() + pool; }
  // count < 0: a frame this rank cannot deliver (no records are looked at)
  void write( uint8_t* at, int64_t pass, int64_t count, const tmc2_patch* records, const int32_t* matches = nullptr,
              const uint8_t* poolBytes = nullptr, size_t poolSize = 0, int64_t tile = 0 ) const {
    int64_t header[4] = {count, int64_t( poolSize ), tile, 0};
    header[kind]      = pass;
    memcpy( at, header, recordsAt() );
    const size_t n = count > 0 ? size_t( count ) : 0;
    if ( n ) memcpy( at + recordsAt(), records, n * sizeof( tmc2_patch ) );
    if ( n && matches ) memcpy( at + matchesAt(), matches, n * 4 );
    if ( poolSize ) memcpy( at + poolAt(), poolBytes, poolSize );
  }
  struct View {  // (bytes, not typed pointers: a block need not be aligned for its records)
    size_t         count = 0, poolSize = 0;
    int64_t        tile = 0;
    const uint8_t *records = nullptr, *matches = nullptr, *pool = nullptr;
    void recordsTo( tmc2_patch* to ) const { if ( count ) memcpy( to, records, count * sizeof( tmc2_patch ) ); }
  };
  bool read( const uint8_t* at, int64_t pass, View& v ) const {  // -> false: not a block of this pass, or of impossible sizes
    int64_t header[4] = {0, 0, 0, 0};
    memcpy( header, at, recordsAt() );
    const int64_t poolSize = kind == kGather ? 0 : header[1];
    if ( header[kind] != pass || header[0] < 0 || header[0] > int64_t( slots ) || poolSize < 0 || poolSize > int64_t( pool ) ) return false;
    v.count = size_t( header[0] ), v.poolSize = size_t( poolSize ), v.tile = header[2];
    v.records = at + recordsAt(), v.matches = at + matchesAt(), v.pool = at + poolAt();
    return true;
  }
};

constexpr int32_t kFailedWord = 0x7FFFFFF0;

// One pass over the frames this process holds, and what its steps share.  comm == nullptr: the frames are the whole GOF -- a world
// of one rank whose meetings are no-ops.  Otherwise they are this rank's share (frame f of the GOF on rank f mod world): the weights
// come from rank 0, the canvas is the maximum over the ranks, the packed records of every frame end on rank 0.
// resume: the frames are segmented and packed already (a pass that ended with "the GOF needs a larger canvas than the buffers hold"):
// the pass starts at the canvas size, from what the packers left in the frames.
struct GofPass {
  tmc2_gof_comm*         comm;
  tmc2_frame**           frames;
  const int32_t*         slotOf;
  int32_t                count, slots;
  const tmc2_gof_config* config;
  uint8_t **             occupancy, **occVideo;
  uint32_t**             blockToPatch;
  uint16_t **            geometryD0, **geometryD1;
  uint8_t**              attribute;
  int32_t                capacityWidth, capacityHeight;
  int32_t *              width, *height;
  int32_t                recordSlots;
  tmc2_patch*            gathered;
  int64_t*               gatheredCounts;
  bool                   resume;
  // what the steps leave for each other
  Pass                 pass;
  bool                 chained = false, guess = false, recordsChain = false;
  std::vector<int>     cores;
  double               weights[3] = {0, 0, 0};
  std::vector<int32_t> heights, guessW, guessH;
  int32_t              W = 0, H = 0;
};

// the frames of one slot in order, slots side by side; a pass that has failed starts no further frame
template <typename Fn>
void perSlot( GofPass& s, Fn fn ) {
  SlotThreads::instance().run( s.slots, s.cores, s.pass, [&]( int sl ) {
    for ( int i = 0; i < s.count; ++i )
      if ( s.slotOf[i] == sl && !s.pass.failed() ) fn( i );
  } );
}

// THE RULE of the sharded pass: a rank that fails locally goes on through every collective of the pass, with a value that says so
// -- nobody is ever left waiting for a rank that has returned.  Here once: the ranks meet in an all-reduce( max ) of `count` words
// whose word 0 carries whether one of them failed (kFailedWord: above every height and size).  -> this rank's own failure with its
// own message, else the collective's, else that another rank failed `phrase`.  Without a communicator: this rank's own failure.
int meet( GofPass& s, int32_t* words, size_t count, const char* what, const char* phrase ) {
  if ( !s.comm ) return s.pass.done();
  if ( s.pass.failed() ) words[0] = kFailedWord;
  const int rc = commMax( s.comm, words, count, what );
  if ( s.pass.failed() ) return s.pass.done();
  if ( rc != TMC2_OK ) return rc;
  if ( words[0] != kFailedWord ) return TMC2_OK;
  t_err = std::string( "tmc2_gof_encode_sharded: another rank's frames " ) + phrase + " (its own call says why)";
  return TMC2_E_STATE;
}

// The final gather: the packed patch records of every frame (the side information the bitstream carries: ~ 100 bytes a patch) to
// rank 0, in list order -- one grouped send / receive per pass.
int commGatherRecords( GofPass& s ) {
  tmc2_gof_comm* comm = s.comm;
  const Block    block{Block::kGather, size_t( s.recordSlots ), 0};
  const size_t   mine = block.bytes() * size_t( s.count ), need = mine * ( comm->rank == 0 ? size_t( comm->world ) + 1 : 1 );
  if ( const int rc = ensureBlocks( comm, need ) ) s.pass.fail( rc, t_err );
  comm->hostBlocks.assign( need, 0 );
  std::vector<tmc2_patch> byIndex, list;
  std::vector<int32_t>    order;
  // (A rank that cannot fill its block -- its pass failed after the rendezvous, or a frame has more patches than the block holds --
  //  STILL takes part in the exchange, with a negative count in the block: the other ranks must not be left waiting in a receive.)
  for ( int i = 0; i < s.count; ++i ) {
    int n = -1;
    if ( !s.pass.failed() ) {
      n = tmc2_frame_patch_count( s.frames[i] );
      if ( n < 0 || n > s.recordSlots ) {
        s.pass.fail( TMC2_E_INVALID, "tmc2_gof_encode_sharded: a frame with " + std::to_string( n ) + " patches, the gather holds " + std::to_string( s.recordSlots ) );
      } else {
        byIndex.resize( size_t( n ) ), list.resize( size_t( n ) ), order.resize( size_t( n ) );
        int rc = tmc2_frame_get_patches( s.frames[i], byIndex.data(), nullptr, nullptr, nullptr );
        if ( rc == TMC2_OK ) rc = tmc2_frame_get_patch_order( s.frames[i], order.data() );
        if ( rc != TMC2_OK ) s.pass.failCall( rc, "tmc2_frame_get_patches" );
        for ( int k = 0; k < n && rc == TMC2_OK; ++k ) list[size_t( k )] = byIndex[size_t( order[size_t( k )] )];
      }
    }
    block.write( comm->hostBlocks.data() + block.bytes() * size_t( i ), comm->passes, s.pass.failed() ? -1 : n, list.data() );
  }
  if ( comm->blocksBytes < need ) {  // (no device buffer: this rank cannot take part at all -- the others must not wait for it)
    breakComm( comm );
    return s.pass.done();
  }
  const int rc = commBlocksToRoot( comm, mine, "ncclSend / ncclRecv( records )" );
  if ( s.pass.failed() ) return s.pass.done();
  if ( rc != TMC2_OK || comm->rank != 0 ) return rc;
  for ( int r = 0; r < comm->world; ++r )
    for ( int i = 0; i < s.count; ++i ) {
      Block::View  v;
      const size_t slot = size_t( r ) * size_t( s.count ) + size_t( i );
      if ( !block.read( comm->hostBlocks.data() + mine * size_t( r + 1 ) + block.bytes() * size_t( i ), comm->passes, v ) ) {
        t_err = "tmc2_gof_encode_sharded: rank " + std::to_string( r ) + " could not deliver the records of its frame " + std::to_string( i ) +
                " (its own call says why)";
        return TMC2_E_STATE;
      }
      if ( s.gatheredCounts ) s.gatheredCounts[slot] = int64_t( v.count );
      if ( s.gathered ) v.recordsTo( s.gathered + slot * size_t( s.recordSlots ) );
    }
  return TMC2_OK;
}

// ---- the packing chains of a sharded GOF (low-delay: spatialConsistencyPackFlexible, PCCEncoder.cpp:1183-1412; random access: +
// performDataAdaptiveGPAMethod, :6821-6971).  They run over ALL frames of the GOF in frame order, microseconds per frame, on patch
// RECORDS ("gather to rank 0 of the per-frame patch table before packing"): every rank sends the records and
// block-occupancy pools of its frames to rank 0 (one grouped send / receive; the block size from an all-reduce of the largest
// frame), rank 0 runs PCCEncoder::placeSegments over them (tmc2_host_place_segments: no device), and every rank gets the packed
// lists of ITS frames back (a 32-byte header broadcast with the canvas and the block size, one grouped send / receive) and
// installs them (tmc2_frame_set_packing).  Rank 0 is left with every frame's records in list order: no gather at the end.
struct ChainResult {
  int32_t W = 0, H = 0;
  // per frame of this rank: the packed list, matches, pool, tile size
  struct Frame {
    std::vector<tmc2_patch> list;
    std::vector<int32_t>    matches;
    std::vector<uint8_t>    occupancy;
    int32_t                 packedW = 0, packedH = 0;
  };
  std::vector<Frame> frames;
};
int chainOverRanks( GofPass& s, ChainResult& out ) {
  tmc2_gof_comm*         comm  = s.comm;
  const tmc2_gof_config& c     = *s.config;
  const int              world = comm->world, count = s.count;
  const size_t           held  = comm->rank == 0 ? size_t( world ) + 1 : 1;  // blocks of `mine` bytes this rank's buffers hold
  // (1) what this rank's frames hold; the largest frame of the GOF sizes everybody's blocks
  std::vector<std::vector<tmc2_patch>> recs( static_cast<size_t>( count ) );
  std::vector<std::vector<uint8_t>>    pools( static_cast<size_t>( count ) );
  int32_t sizes[3] = {0, 0, 0};  // failed?, most patches of a frame, largest pool of a frame
  for ( int i = 0; i < count && !s.pass.failed(); ++i ) {
    const int n = tmc2_frame_patch_count( s.frames[i] );
    int64_t   depth = 0, occ = 0;
    if ( n < 0 || tmc2_frame_patch_pool_sizes( s.frames[i], &depth, &occ ) != TMC2_OK || occ < 0 || occ > 0x3FFFFFFF ) {
      s.pass.failCall( TMC2_E_STATE, "tmc2_frame_patch_pool_sizes" );
      break;
    }
    recs[size_t( i )].resize( size_t( n ) ), pools[size_t( i )].resize( size_t( occ ) );
    if ( const int rc = tmc2_frame_get_patches( s.frames[i], recs[size_t( i )].data(), nullptr, nullptr, pools[size_t( i )].data() ) ) {
      s.pass.failCall( rc, "tmc2_frame_get_patches" );
      break;
    }
    sizes[1] = std::max( sizes[1], int32_t( n ) ), sizes[2] = std::max( sizes[2], int32_t( occ ) );
  }
  // (every rank leaves here, together)
  if ( const int rc = meet( s, sizes, 3, "ncclAllReduce( records of the largest frame, max )", "failed before the packing chain" ) ) return rc;
  if ( sizes[1] > s.recordSlots ) {
    t_err = "tmc2_gof_encode_sharded: a frame with " + std::to_string( sizes[1] ) + " patches, the records hold " + std::to_string( s.recordSlots );
    return TMC2_E_INVALID;
  }
  const size_t slotsN = size_t( std::max( sizes[1], 1 ) );
  const Block  in{Block::kToRoot, slotsN, roundUp( size_t( sizes[2] ), 64 )};
  const size_t inMine = in.bytes() * size_t( count );
  // (2) records + pools -> rank 0
  int rc = ensureBlocks( comm, inMine * held );
  if ( rc != TMC2_OK ) {  // (cannot take part: the others must not wait)
    breakComm( comm );
    return rc;
  }
  comm->hostBlocks.assign( inMine * held, 0 );
  for ( int i = 0; i < count; ++i )
    in.write( comm->hostBlocks.data() + in.bytes() * size_t( i ), comm->passes, int64_t( recs[size_t( i )].size() ), recs[size_t( i )].data(), nullptr,
              pools[size_t( i )].data(), pools[size_t( i )].size() );
  rc = commBlocksToRoot( comm, inMine, "ncclSend / ncclRecv( records for the packing chain )" );
  if ( rc != TMC2_OK ) return rc;
  // (3) rank 0: PCCEncoder::placeSegments over the GOF in frame order (frame f = slot f / world of rank f mod world)
  const int            gofFrames = count * world;
  int32_t              header[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // status, W, H, bytes of the largest packed pool
  std::vector<int32_t> counts, matches, widths, heights;
  std::vector<tmc2_patch> all;
  std::vector<uint8_t>    occOut;
  std::vector<int64_t>    outBase;
  if ( comm->rank == 0 ) {
    std::vector<uint8_t> occIn;
    std::vector<int64_t> inBase;
    counts.resize( size_t( gofFrames ) ), inBase.resize( size_t( gofFrames ) ), outBase.resize( size_t( gofFrames ) + 1 );
    widths.resize( size_t( gofFrames ) ), heights.resize( size_t( gofFrames ) );
    bool ok = true;
    for ( int f = 0; f < gofFrames && ok; ++f ) {
      Block::View v;
      ok = in.read( comm->hostBlocks.data() + inMine * size_t( f % world + 1 ) + in.bytes() * size_t( f / world ), comm->passes, v );
      if ( !ok ) break;
      counts[size_t( f )] = int32_t( v.count ), inBase[size_t( f )] = int64_t( occIn.size() );
      all.resize( all.size() + v.count );
      v.recordsTo( all.data() + all.size() - v.count );
      occIn.insert( occIn.end(), v.pool, v.pool + v.poolSize );
    }
    if ( !ok ) {
      header[0] = kFailedWord;
      s.pass.fail( TMC2_E_STATE, "tmc2_gof_encode_sharded: a rank delivered a block of another pass or of impossible sizes" );
    } else {
      // (random access: a tracked patch grows to the box of its track's union -- never beyond the largest box of the GOF in either direction)
      int64_t maxU0 = 1, maxV0 = 1;
      for ( const tmc2_patch& p : all ) maxU0 = std::max<int64_t>( maxU0, p.sizeU0 ), maxV0 = std::max<int64_t>( maxV0, p.sizeV0 );
      const int64_t cap = c.packing == 2 ? int64_t( all.size() ) * maxU0 * maxV0 : int64_t( occIn.size() );
      occOut.assign( size_t( std::max<int64_t>( cap, 1 ) ), 0 ), matches.assign( std::max<size_t>( all.size(), 1 ), -1 );
      const int prc = tmc2_host_place_segments( gofFrames, counts.data(), all.data(), occIn.data(), inBase.data(), c.packing, c.minimumImageWidth,
                                                c.minimumImageHeight, 2, 1.0, matches.data(), occOut.data(), cap, outBase.data(), widths.data(),
                                                heights.data() );
      int32_t tileW = c.minimumImageWidth, tileH = 0;
      for ( int f = 0; f < gofFrames; ++f ) tileW = std::max( tileW, widths[size_t( f )] ), tileH = std::max( tileH, heights[size_t( f )] );
      if ( c.packing == 2 ) tileH = std::max( tileH, c.minimumImageHeight );
      int32_t   W = 0, H = 0;
      const int crc = prc != TMC2_OK ? prc : tmc2_encoder_canvas_size( &tileH, 1, tileW, c.minimumImageWidth, c.minimumImageHeight, &W, &H );
      if ( crc != TMC2_OK ) {
        header[0] = kFailedWord;
        s.pass.failCall( crc, prc != TMC2_OK ? "tmc2_host_place_segments" : "tmc2_encoder_canvas_size" );
      } else {
        int64_t largest = 0;
        for ( int f = 0; f < gofFrames; ++f ) largest = std::max( largest, outBase[size_t( f ) + 1] - outBase[size_t( f )] );
        header[1] = W, header[2] = H, header[3] = int32_t( largest );
      }
    }
  }
  rc = commBroadcast( comm, header, 8, kNcclInt32, 4, "ncclBroadcast( canvas of the GOF )" );
  if ( rc != TMC2_OK ) return rc;
  if ( header[0] != 0 ) {
    if ( s.pass.failed() ) return s.pass.done();
    t_err = "tmc2_gof_encode_sharded: the packing chain failed on rank 0 (its own call says why)";
    return TMC2_E_STATE;
  }
  // (4) the packed lists back to the ranks that hold the frames
  const Block  back{Block::kFromRoot, slotsN, roundUp( size_t( header[3] ), 64 )};
  const size_t outMine = back.bytes() * size_t( count );
  rc = ensureBlocks( comm, outMine * held );
  if ( rc != TMC2_OK ) {
    breakComm( comm );
    return rc;
  }
  comm->hostBlocks.assign( outMine * ( comm->rank == 0 ? size_t( world ) : 1 ), 0 );
  if ( comm->rank == 0 ) {
    size_t first = 0;
    for ( int f = 0; f < gofFrames; ++f ) {
      const size_t n = size_t( counts[size_t( f )] ), slot = size_t( f % world ) * size_t( count ) + size_t( f / world );
      back.write( comm->hostBlocks.data() + outMine * size_t( f % world ) + back.bytes() * size_t( f / world ), comm->passes, int64_t( n ),
                  all.data() + first, matches.data() + first, occOut.data() + outBase[size_t( f )], size_t( outBase[size_t( f ) + 1] - outBase[size_t( f )] ),
                  ( int64_t( widths[size_t( f )] ) << 32 ) | uint32_t( heights[size_t( f )] ) );
      if ( s.gatheredCounts ) s.gatheredCounts[slot] = int64_t( n );
      if ( s.gathered && n ) memcpy( s.gathered + slot * size_t( s.recordSlots ), all.data() + first, n * sizeof( tmc2_patch ) );
      first += n;
    }
  }
  rc = commBlocksFromRoot( comm, outMine, "ncclSend / ncclRecv( packed lists )" );
  if ( rc != TMC2_OK ) return rc;
  out.W = header[1], out.H = header[2];
  out.frames.resize( size_t( count ) );
  for ( int i = 0; i < count; ++i ) {
    Block::View v;
    if ( !back.read( comm->hostBlocks.data() + back.bytes() * size_t( i ), comm->passes, v ) ) {
      t_err = "tmc2_gof_encode_sharded: the packed list of frame " + std::to_string( i ) + " did not arrive";
      return TMC2_E_STATE;
    }
    ChainResult::Frame& fr = out.frames[size_t( i )];
    fr.list.resize( v.count ), fr.matches.resize( v.count ), fr.occupancy.assign( v.pool, v.pool + v.poolSize );
    v.recordsTo( fr.list.data() );
    if ( v.count ) memcpy( fr.matches.data(), v.matches, v.count * 4 );
    fr.packedW = int32_t( v.tile >> 32 ), fr.packedH = int32_t( v.tile & 0xFFFFFFFF );
  }
  return TMC2_OK;
}

// Where rank 0 publishes the communicator's id when the caller names no file: /dev/shm/tmc2_gof_id_<uid>_$MASTER_PORT.  The port
// is what tells two jobs of one node apart, so several ranks without it are refused.
int defaultRendezvous( int worldSize, std::string& path ) {
  const char* port = getenv( "MASTER_PORT" );
  if ( !port && worldSize > 1 ) {
    t_err = "tmc2_gof_comm_create: no rendezvous file was named and MASTER_PORT is not set: two jobs on this node would read each other's id";
    return TMC2_E_INVALID;
  }
  path = "/dev/shm/tmc2_gof_id_" + std::to_string( long( getuid() ) ) + "_" + ( port ? port : "0" );
  return TMC2_OK;
}
// seconds since the epoch at which this process started (/proc/self/stat field 22 in clock ticks since boot + /proc/stat btime);
// 0 if it cannot be read
double processStart() {
  std::ifstream st( "/proc/self/stat" ), boot( "/proc/stat" );
  std::string   line;
  if ( !std::getline( st, line ) ) return 0.0;
  const size_t close = line.rfind( ')' );
  if ( close == std::string::npos ) return 0.0;
  unsigned long long ticks = 0;
  {
    const char* p = line.c_str() + close + 1;
    for ( int field = 3; field <= 22; ++field ) {
      while ( *p == ' ' ) ++p;
      if ( field == 22 ) ticks = strtoull( p, nullptr, 10 );
      while ( *p && *p != ' ' ) ++p;
    }
  }
  double btime = 0.0;
  while ( std::getline( boot, line ) )
    if ( line.compare( 0, 6, "btime " ) == 0 ) btime = atof( line.c_str() + 6 );
  const long hz = sysconf( _SC_CLK_TCK );
  return btime > 0.0 && hz > 0 ? btime + double( ticks ) / double( hz ) : 0.0;
}
constexpr char kIdMagic[8] = {'t', 'm', 'c', '2', 'i', 'd', '0', '1'};
}  // namespace

extern "C" int tmc2_gof_comm_create( int rank, int worldSize, tmc2_ctx* ctx, const char* rendezvous, tmc2_gof_comm** out ) {
  if ( !out ) return TMC2_E_INVALID;
  *out = nullptr;
  if ( rank < 0 || worldSize < 1 || rank >= worldSize || !ctx ) {
    t_err = "tmc2_gof_comm_create: invalid argument";
    return TMC2_E_INVALID;
  }
  // (every failure below goes through tmc2_gof_comm_destroy: the RCCL communicator, the device words and the library handle with it)
  std::unique_ptr<tmc2_gof_comm, void ( * )( tmc2_gof_comm* )> owner( new tmc2_gof_comm(), tmc2_gof_comm_destroy );
  tmc2_gof_comm*                                                comm = owner.get();
  comm->rank = rank, comm->world = worldSize, comm->ctx = ctx;
  if ( const char* t = getenv( "TMC2_GOF_COLLECTIVE_TIMEOUT" ) ) comm->timeoutSeconds = atof( t );
  std::string why;
  if ( !comm->rccl.load( why ) ) {
    t_err = "tmc2_gof_comm_create: RCCL not available (" + why + ")";
    return TMC2_E_UNSUPPORTED;
  }
  HIP_TRY( tmc2_ctx_make_current( ctx ), "tmc2_ctx_make_current" );
  // The 128-byte id of the communicator: rank 0 makes it and publishes it in a file (same node: /dev/shm), the others wait for it.
  // The file is created exclusively (O_EXCL | O_NOFOLLOW, mode 0600: no symbolic link is followed, nobody else's file is reused)
  // after whatever an earlier run left under the name has been removed, and renamed into place complete.  A reader accepts only a
  // complete file of ITS user that is not older than the reader's own process: what a crashed run of the same port left behind
  // was written before this job's processes were started.
  std::string path = rendezvous ? rendezvous : "";
  if ( path.empty() )
    if ( const int rc = defaultRendezvous( worldSize, path ) ) return rc;
  NcclId id{};
  if ( rank == 0 ) {
    if ( const int rc = comm->rccl.GetUniqueId( &id ) ) return ncclFailed( comm, rc, "ncclGetUniqueId" );
    if ( worldSize > 1 ) {
      const std::string tmp = path + ".tmp." + std::to_string( long( getpid() ) );
      (void)unlink( path.c_str() ), (void)unlink( tmp.c_str() );
      const int fd = open( tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600 );
      bool      ok = fd >= 0;
      ok = ok && write( fd, kIdMagic, sizeof( kIdMagic ) ) == ssize_t( sizeof( kIdMagic ) );
      ok = ok && write( fd, id.internal, sizeof( id.internal ) ) == ssize_t( sizeof( id.internal ) );
      if ( fd >= 0 ) ok = ( close( fd ) == 0 ) && ok;
      if ( !ok || rename( tmp.c_str(), path.c_str() ) != 0 ) {
        (void)unlink( tmp.c_str() );
        t_err = "tmc2_gof_comm_create: cannot publish the communicator id in " + path;
        return TMC2_E_INVALID;
      }
    }
  } else {
    const double started = processStart();
    const auto   limit   = std::chrono::steady_clock::now() + std::chrono::seconds( 120 );
    for ( ;; ) {
      const int fd = open( path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC );
      if ( fd >= 0 ) {
        struct stat info;
        char        magic[sizeof( kIdMagic )];
        const bool  mine  = fstat( fd, &info ) == 0 && S_ISREG( info.st_mode ) && info.st_uid == getuid();
        const bool  fresh = mine && ( started <= 0.0 || double( info.st_mtim.tv_sec ) + 1e-9 * double( info.st_mtim.tv_nsec ) + 1.0 >= started );
        const bool  whole = fresh && read( fd, magic, sizeof( magic ) ) == ssize_t( sizeof( magic ) ) && memcmp( magic, kIdMagic, sizeof( magic ) ) == 0 &&
                           read( fd, id.internal, sizeof( id.internal ) ) == ssize_t( sizeof( id.internal ) );
        close( fd );
        if ( whole ) break;
      }
      if ( std::chrono::steady_clock::now() > limit ) {
        t_err = "tmc2_gof_comm_create: rank 0 never published the communicator id in " + path + " (a file that is older than this process, "
                "another user's, or incomplete does not count)";
        return TMC2_E_STATE;
      }
      std::this_thread::sleep_for( std::chrono::milliseconds( 5 ) );
    }
  }
  if ( const int rc = comm->rccl.CommInitRank( &comm->comm, worldSize, id, rank ) ) return ncclFailed( comm, rc, "ncclCommInitRank" );
  HIP_TRY( tmc2_ctx_device_alloc( ctx, 64, &comm->dSmall ), "tmc2_ctx_device_alloc" );
  int32_t probe = 100 + rank;  // pre-flight: one collective through the new communicator, checked
  {
    const int rc = commMax( comm, &probe, 1, "ncclAllReduce( height, max )" );
    if ( rank == 0 && worldSize > 1 ) unlink( path.c_str() );  // (every rank has read it -- or will never: the all-reduce is over)
    if ( rc != TMC2_OK ) return rc;
  }
  if ( probe != 100 + worldSize - 1 ) {
    t_err = "tmc2_gof_comm_create: the pre-flight all-reduce gave " + std::to_string( probe );
    return TMC2_E_STATE;
  }
  *out = owner.release();
  return TMC2_OK;
}

extern "C" void tmc2_gof_comm_destroy( tmc2_gof_comm* comm ) {
  if ( !comm ) return;
  if ( comm->dSmall ) (void)tmc2_ctx_device_free( comm->ctx, comm->dSmall );
  if ( comm->dBlocks ) (void)tmc2_ctx_device_free( comm->ctx, comm->dBlocks );
  if ( comm->comm ) (void)comm->rccl.CommDestroy( comm->comm );
  if ( comm->rccl.lib ) dlclose( comm->rccl.lib );
  delete comm;
}

// ---- the steps of a pass, in the order encodeGof() takes them.  A step returns TMC2_OK to go on, anything else to leave the
// pass with -- and where there are ranks every rank leaves at the same step (meet(), the weights, the chain's header).
namespace {
int checkArguments( GofPass& s ) {
  if ( !s.frames || !s.slotOf || !s.config || s.count <= 0 || s.slots <= 0 || !s.width || !s.height ) {
    t_err = "tmc2_gof_encode: invalid argument";
    return TMC2_E_INVALID;
  }
  for ( int i = 0; i < s.count; ++i )
    if ( !s.frames[i] || s.slotOf[i] < 0 || s.slotOf[i] >= s.slots ) {
      t_err = "tmc2_gof_encode: frame " + std::to_string( i ) + " is null or on a slot outside [0, " + std::to_string( s.slots ) + ")";
      return TMC2_E_INVALID;
    }
  const tmc2_gof_config& c = *s.config;
  if ( c.packing < 0 || c.packing > 2 ) {
    t_err = "tmc2_gof_encode: packing " + std::to_string( c.packing ) + " (0 all-intra, 1 low-delay, 2 random-access)";
    return TMC2_E_INVALID;
  }
  if ( s.comm ) {
    if ( const int rc = refuseBroken( s.comm ) ) return rc;
    ++s.comm->passes;
  }
  // several ranks under a chained condition: the chain runs on rank 0 over the records (TMC2_GOF_RECORDS_CHAIN=1 forces that route
  // for a communicator of one rank too: the GPU tier runs it that way on a one-GPU box)
  const char* forced = getenv( "TMC2_GOF_RECORDS_CHAIN" );
  s.chained = c.packing != 0, s.guess = !s.chained && c.guessCanvas != 0;
  s.recordsChain = s.comm && s.chained && ( s.comm->world > 1 || ( forced && atoi( forced ) != 0 ) );
  s.cores = coresByCacheDomain();
  s.heights.assign( size_t( s.count ), 0 ), s.guessW.assign( size_t( s.count ), 0 ), s.guessH.assign( size_t( s.count ), 0 );
  const bool anyOut = s.occupancy || s.occVideo || s.blockToPatch || s.geometryD0 || s.geometryD1 || s.attribute;
  if ( !anyOut ) s.capacityWidth = s.capacityHeight = INT32_MAX;  // (nothing leaves the device: no capacity to respect)
  return TMC2_OK;
}

// every frame reset, S0 on frame 0 of the GOF (rank 0's first), its weights to every rank
int resetAndWeights( GofPass& s ) {
  if ( s.resume ) return TMC2_OK;
  for ( int i = 0; i < s.count && !s.pass.failed(); ++i )
    if ( const int rc = tmc2_frame_reset( s.frames[i] ) ) s.pass.failCall( rc, "tmc2_frame_reset" );
  const bool root = !s.comm || s.comm->rank == 0;
  if ( root && !s.pass.failed() )
    if ( const int rc = tmc2_weight_normal( s.frames[0], s.config->geometryBitDepth3D, 0.6, s.weights ) ) s.pass.failCall( rc, "tmc2_weight_normal" );
  if ( !s.comm ) return s.pass.done();
  // (no axis weight is negative: from a negative one the other ranks learn that rank 0 has no pass to offer)
  if ( root && s.pass.failed() ) s.weights[0] = s.weights[1] = s.weights[2] = -1.0;
  if ( const int rc = commBroadcast( s.comm, s.weights, 3, kNcclFloat64, 8, "ncclBroadcast( weights )" ) ) s.pass.fail( rc, "tmc2_gof_encode_sharded: " + t_err );
  if ( s.weights[0] < 0.0 ) {  // (the same on every rank: all leave here)
    if ( s.pass.failed() ) return s.pass.done();
    t_err = "tmc2_gof_encode_sharded: rank 0 could not start the pass (its own call says why)";
    return TMC2_E_STATE;
  }
  return s.comm->broken ? s.pass.done() : TMC2_OK;
}

// what follows the packing of one frame, on a canvas of W x H: S12-S22 and the copies of its finished canvases
void images( GofPass& s, int i, int32_t W, int32_t H ) {
  if ( W > s.capacityWidth || H > s.capacityHeight ) return;  // (refused after the rendezvous, with the size the GOF needs)
  tmc2_frame* f = s.frames[i];
  GOF_TRY( tmc2_encoder_generate_geometry_images( f, W, H, s.config->occupancyPrecision ) );
  GOF_TRY( tmc2_encoder_generate_attribute_images( f ) );
  auto at = []( auto** arr, int k ) { return arr ? arr[k] : nullptr; };
  if ( s.occupancy || s.occVideo || s.blockToPatch || s.geometryD0 || s.geometryD1 )
    GOF_TRY( tmc2_frame_get_geometry_images( f, at( s.occupancy, i ), at( s.occVideo, i ), at( s.blockToPatch, i ), at( s.geometryD0, i ),
                                             at( s.geometryD1, i ) ) );
  if ( s.attribute && s.attribute[i] ) GOF_TRY( tmc2_frame_get_attribute_images( f, s.attribute[i] ) );
}

// S1-S9 per frame and, all-intra, the frame's own packing.  With guessCanvas a frame does not wait for the others: it goes through
// its whole chain on the canvas ITS OWN packed height gives (with the CTC sequences: the minimum canvas, for every frame); the
// rendezvous then only compares, and a frame whose guess was short rasterises again on the common canvas (same bytes as the
// two-phase order: the images depend on the final size only).
void segmentAndPack( GofPass& s ) {
  if ( s.resume || s.pass.failed() ) return;
  const tmc2_gof_config&      c      = *s.config;
  const tmc2_segmenter_params params = ctcParams( c, s.weights );
  perSlot( s, [&]( int i ) {
    int32_t& h = s.heights[size_t( i )];
    GOF_TRY( tmc2_segmenter_compute( s.frames[i], &params ) );
    if ( s.chained ) return;
    GOF_TRY( tmc2_encoder_pack_flexible( s.frames[i], c.minimumImageWidth, 2, 1.0, &h ) );
    if ( !s.guess ) return;
    GOF_TRY( tmc2_encoder_canvas_size( &h, 1, c.minimumImageWidth, c.minimumImageWidth, c.minimumImageHeight, &s.guessW[size_t( i )], &s.guessH[size_t( i )] ) );
    images( s, i, s.guessW[size_t( i )], s.guessH[size_t( i )] );
  } );
}

// the canvas of a GOF from its widest and tallest tile (a function of the GOF's numbers: the same on every rank)
int canvasOf( GofPass& s, int32_t tileW, int32_t tileH ) {
  const tmc2_gof_config& c = *s.config;
  if ( const int rc = tmc2_encoder_canvas_size( &tileH, 1, tileW, c.minimumImageWidth, c.minimumImageHeight, &s.W, &s.H ) ) s.pass.failCall( rc, "tmc2_encoder_canvas_size" );
  return s.pass.done();
}

// route 1, resume: the frames are packed -- the tiles the packers left (tmc2_frame_get_packed_size)
int canvasFromTiles( GofPass& s ) {
  const tmc2_gof_config& c = *s.config;
  int32_t words[3] = {0, c.minimumImageWidth, 0};  // failed?, widest tile, tallest tile
  for ( int i = 0; i < s.count; ++i ) {
    int32_t   pw = 0, ph = 0;
    const int rc = tmc2_frame_get_packed_size( s.frames[i], &pw, &ph );
    if ( rc != TMC2_OK ) s.pass.failCall( rc, "tmc2_frame_get_packed_size" );
    else if ( pw <= 0 ) s.pass.fail( TMC2_E_STATE, "tmc2_gof_encode_resume: a frame is not packed (the pass to resume must have ended with 'the GOF needs a larger canvas')" );
    words[1] = std::max( words[1], pw ), words[2] = std::max( words[2], ph );
  }
  if ( c.packing == 2 ) words[2] = std::max( words[2], c.minimumImageHeight );
  if ( const int rc = meet( s, words, 3, "ncclAllReduce( tile of the GOF, max )", "are not packed" ) ) return rc;
  return canvasOf( s, words[1], words[2] );
}

// route 2, several ranks under a chained condition: records to rank 0, the chain there, the packed lists back
int canvasThroughChain( GofPass& s ) {
  ChainResult chain;
  if ( const int rc = chainOverRanks( s, chain ) ) return rc;  // (every rank leaves at the same place: chainOverRanks)
  s.W = chain.W, s.H = chain.H;
  // (installed before the buffers are looked at: a pass that ends with "the GOF needs a larger canvas" leaves its frames packed)
  perSlot( s, [&]( int i ) {
    const ChainResult::Frame& fr = chain.frames[size_t( i )];
    GOF_TRY( tmc2_frame_set_packing( s.frames[i], fr.list.data(), int( fr.list.size() ), fr.matches.data(), fr.occupancy.data(),
                                     int64_t( fr.occupancy.size() ), fr.packedW, fr.packedH ) );
  } );
  return TMC2_OK;
}

// the packing chain over frames that all live here, in frame order on the calling thread -> the widest tile
int32_t chainHere( GofPass& s ) {
  const tmc2_gof_config& c = *s.config;
  int32_t                tileW = c.minimumImageWidth;
  auto once = [&]( int rc, const char* what ) {
    if ( rc != TMC2_OK ) s.pass.failCall( rc, what );
    return rc == TMC2_OK;
  };
  bool ok = once( tmc2_encoder_pack_flexible( s.frames[0], c.minimumImageWidth, 2, 1.0, &s.heights[0] ), "tmc2_encoder_pack_flexible" );
  for ( int i = 1; i < s.count && ok; ++i )
    ok = once( tmc2_encoder_pack_spatial_consistency( s.frames[i], s.frames[i - 1], c.minimumImageWidth, 2, 1.0, &s.heights[size_t( i )] ),
               "tmc2_encoder_pack_spatial_consistency" );
  if ( ok && c.packing == 2 ) {
    std::vector<int32_t> widths( static_cast<size_t>( s.count ), 0 );
    ok = once( tmc2_encoder_global_patch_allocation( s.frames, s.count, c.minimumImageWidth, c.minimumImageHeight, widths.data(), s.heights.data() ),
               "tmc2_encoder_global_patch_allocation" );
    for ( int i = 0; i < s.count && ok; ++i ) {
      tileW                  = std::max( tileW, widths[size_t( i )] );
      s.heights[size_t( i )] = std::max( s.heights[size_t( i )], c.minimumImageHeight );
    }
  } else {
    for ( int i = 0; i < s.count && ok; ++i ) {
      int32_t pw = 0;
      ok         = once( tmc2_frame_get_packed_size( s.frames[i], &pw, nullptr ), "tmc2_frame_get_packed_size" );
      tileW      = std::max( tileW, pw );
    }
  }
  return tileW;
}

// route 3: the heights the packers gave (all-intra: per frame, above; chained: the chain over the frames here), and -- the one
// number the ranks of an all-intra GOF share -- their maximum over the ranks
int canvasFromHeights( GofPass& s ) {
  const int32_t tileW = s.chained && !s.pass.failed() ? chainHere( s ) : s.config->minimumImageWidth;
  int32_t       gofH  = 0;
  for ( int i = 0; i < s.count; ++i ) gofH = std::max( gofH, s.heights[size_t( i )] );
  if ( const int rc = meet( s, &gofH, 1, "ncclAllReduce( height, max )", "failed before the rendezvous" ) ) return rc;
  return canvasOf( s, tileW, gofH );
}

int refuseACanvasBeyondTheBuffers( GofPass& s ) {  // (the same on every rank: W and H are the GOF's)
  *s.width = s.W, *s.height = s.H;
  if ( s.W <= s.capacityWidth && s.H <= s.capacityHeight ) return TMC2_OK;
  char msg[160];
  std::snprintf( msg, sizeof( msg ), "tmc2_gof_encode: the GOF needs a %d x %d canvas, the buffers hold %d x %d", s.W, s.H, s.capacityWidth, s.capacityHeight );
  t_err = msg;
  return TMC2_E_INVALID;
}

// from here the frames are independent: images, attribute images, copies, each on its slot
void imagesAndCopies( GofPass& s ) {
  perSlot( s, [&]( int i ) {
    if ( s.guess && !s.resume && s.guessW[size_t( i )] == s.W && s.guessH[size_t( i )] == s.H ) return;  // (already there)
    images( s, i, s.W, s.H );
  } );
}

// (a pass that failed after the rendezvous still takes part in the exchange.)  A chained GOF left every record on rank 0 already;
// what its ranks still owe each other is whether the pass held.
int closePass( GofPass& s ) {
  if ( s.comm && ( !s.recordsChain || s.resume ) ) return commGatherRecords( s );
  int32_t bad = 0;
  return meet( s, &bad, 1, "ncclAllReduce( status of the pass, max )", "failed after the rendezvous" );
}

int encodeGof( GofPass& s ) {
  t_err.clear();
  if ( const int rc = checkArguments( s ) ) return rc;
  if ( const int rc = resetAndWeights( s ) ) return rc;
  segmentAndPack( s );
  if ( const int rc = s.resume ? canvasFromTiles( s ) : s.recordsChain ? canvasThroughChain( s ) : canvasFromHeights( s ) ) return rc;
  if ( const int rc = refuseACanvasBeyondTheBuffers( s ) ) return rc;
  imagesAndCopies( s );
  return closePass( s );
}

// (nothing may leave through the C boundary but a status: what the CALLING thread throws -- a std::bad_alloc, a std::system_error
//  of the thread pool -- is caught here; what a slot thread throws fails the pass where it is caught, SlotThreads::run)
int guarded( GofPass& s ) {
  try {
    return encodeGof( s );
  } catch ( const std::exception& e ) {
    t_err = std::string( "tmc2_gof_encode: " ) + e.what();
  } catch ( ... ) {
    t_err = "tmc2_gof_encode: unknown exception";
  }
  return TMC2_E_STATE;
}
}  // namespace

// the entries: one pass each, told apart by the communicator (none: the frames are the whole GOF) and by where the pass starts
static int run( tmc2_gof_comm* comm, bool resume, tmc2_frame** frames, const int32_t* slotOf, int32_t count, int32_t slots,
                const tmc2_gof_config* config, uint8_t** occupancy, uint8_t** occVideo, uint32_t** blockToPatch, uint16_t** geometryD0,
                uint16_t** geometryD1, uint8_t** attribute, int32_t capacityWidth, int32_t capacityHeight, int32_t* width, int32_t* height,
                int32_t recordSlots = 0, tmc2_patch* gathered = nullptr, int64_t* gatheredCounts = nullptr ) {
  GofPass s{comm,      frames,        slotOf,         count, slots,  config,      occupancy, occVideo,       blockToPatch, geometryD0, geometryD1,
            attribute, capacityWidth, capacityHeight, width, height, recordSlots, gathered,  gatheredCounts, resume};
  return guarded( s );
}
static int shardedArguments( tmc2_gof_comm* comm, int32_t recordSlots ) {  // -> what the sharded entries refuse before the pass
  if ( comm && recordSlots > 0 ) return TMC2_OK;
  t_err = "tmc2_gof_encode_sharded: invalid argument";
  return TMC2_E_INVALID;
}

extern "C" int tmc2_gof_encode( tmc2_frame** frames, const int32_t* slotOf, int32_t count, int32_t slots, const tmc2_gof_config* config,
                                uint8_t** occupancy, uint8_t** occVideo, uint32_t** blockToPatch, uint16_t** geometryD0,
                                uint16_t** geometryD1, uint8_t** attribute, int32_t capacityWidth, int32_t capacityHeight,
                                int32_t* width, int32_t* height ) {
  return run( nullptr, false, frames, slotOf, count, slots, config, occupancy, occVideo, blockToPatch, geometryD0, geometryD1, attribute,
              capacityWidth, capacityHeight, width, height );
}

extern "C" int tmc2_gof_encode_resume( tmc2_frame** frames, const int32_t* slotOf, int32_t count, int32_t slots, const tmc2_gof_config* config,
                                       uint8_t** occupancy, uint8_t** occVideo, uint32_t** blockToPatch, uint16_t** geometryD0,
                                       uint16_t** geometryD1, uint8_t** attribute, int32_t capacityWidth, int32_t capacityHeight,
                                       int32_t* width, int32_t* height ) {
  return run( nullptr, true, frames, slotOf, count, slots, config, occupancy, occVideo, blockToPatch, geometryD0, geometryD1, attribute,
              capacityWidth, capacityHeight, width, height );
}

extern "C" int tmc2_gof_encode_sharded( tmc2_gof_comm* comm, tmc2_frame** frames, const int32_t* slotOf, int32_t count, int32_t slots,
                                        const tmc2_gof_config* config, uint8_t** occupancy, uint8_t** occVideo, uint32_t** blockToPatch,
                                        uint16_t** geometryD0, uint16_t** geometryD1, uint8_t** attribute, int32_t capacityWidth,
                                        int32_t capacityHeight, int32_t* width, int32_t* height, int32_t recordSlots, tmc2_patch* gathered,
                                        int64_t* gatheredCounts ) {
  if ( const int rc = shardedArguments( comm, recordSlots ) ) return rc;
  return run( comm, false, frames, slotOf, count, slots, config, occupancy, occVideo, blockToPatch, geometryD0, geometryD1, attribute,
              capacityWidth, capacityHeight, width, height, recordSlots, gathered, gatheredCounts );
}

extern "C" int tmc2_gof_encode_sharded_resume( tmc2_gof_comm* comm, tmc2_frame** frames, const int32_t* slotOf, int32_t count, int32_t slots,
                                               const tmc2_gof_config* config, uint8_t** occupancy, uint8_t** occVideo,
                                               uint32_t** blockToPatch, uint16_t** geometryD0, uint16_t** geometryD1, uint8_t** attribute,
                                               int32_t capacityWidth, int32_t capacityHeight, int32_t* width, int32_t* height,
                                               int32_t recordSlots, tmc2_patch* gathered, int64_t* gatheredCounts ) {
  if ( const int rc = shardedArguments( comm, recordSlots ) ) return rc;
  return run( comm, true, frames, slotOf, count, slots, config, occupancy, occVideo, blockToPatch, geometryD0, geometryD1, attribute,
              capacityWidth, capacityHeight, width, height, recordSlots, gathered, gatheredCounts );
}
