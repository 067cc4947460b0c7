// Paged KV-cache block allocator with hash-chained prefix caching.
//
// Blocks are 16-token pages shared by all layers (one block id addresses the
// same page in every layer's K and V pools). A block that is full and whose KV
// has been computed is registered under hash(parent_hash, its 16 tokens); when
// its last user releases it, it stays resident among the evictable blocks so a later
// request with the same prefix (same task text, same prompt template head) reuses it
// without recomputation. Fresh allocations take truly free blocks first and evict
// cached blocks only when needed, segmented-LRU: blocks never reused since they were
// computed (a call's private template/dynamic text) go first, oldest first; blocks that
// were reused at least once (a task's shared prefix) are protected (up to half the
// pool; the oldest protected block is demoted when it overflows). With plain LRU the
// 64-worker bench lost 6 points of prefix-cache hits once eviction started.
//
// Donor index (partial-block reuse): every registered block is also listed under its PARENT's
// hash, with the number of leading slots whose KV is valid (16 for a full block, the prompt's
// tail length for the last, partly filled block of a finished prefill). A prompt that leaves
// the hash chain inside a block asks match_head() for the listed block sharing the longest
// head with it and copies those slots (csrc/ops/kv_copy.hip) instead of computing them. A
// partial tail block is evictable like a hashed block once its last user releases it.
//
// Host tier (host_slots > 0): a second, host-resident directory hash -> slot under the device
// cache. Evicting a hashed full block lists a spill (block, slot) unless its hash is already in
// the directory (the tier is inclusive: a restored block is never spilled twice); a chain that
// continues into the directory gets a fresh device block per host hit and a fill (slot, block).
// The manager only plans the moves: the caller takes them (take_moves) and runs every spill,
// then every fill, before the device blocks are read or written again. A slot named by a move
// not yet taken is pinned: it is neither evicted from the tier nor given to another spill.
// Partial tail donors are not spilled.
#pragma once
#include <cstdint>
#include <list>
#include <unordered_map>
#include <vector>

namespace rt {

uint64_t hash_block(uint64_t parent, const int32_t* tokens, int n);

struct KvMove {
  int32_t block, slot;  // device block, host slot
};

class BlockManager {
 public:
  BlockManager(int32_t num_blocks, int32_t block_size, bool prefix_caching, int32_t host_slots = 0);
  int32_t block_size() const { return block_size_; }
  int32_t num_blocks() const { return num_blocks_; }
  int32_t num_free() const { return (int32_t)(free_list_.size() + lru_[0].size() + lru_[1].size()); }
  int32_t num_cached() const { return (int32_t)cache_.size(); }
  bool allocate(int32_t n, std::vector<int32_t>& out);
  void release(int32_t block);
  // Prefix lookup: returns the block holding exactly `tokens` under `hash`, with
  // its reference taken, or -1.
  int32_t lookup(uint64_t hash, const int32_t* tokens);
  // `parent`: the hash of the block before it (0 for a sequence's first block); the block is
  // listed under it as a donor of all block_size slots
  void register_block(int32_t block, uint64_t hash, const int32_t* tokens, uint64_t parent = 0);
  // List `block`, whose first `fill` slots (0 < fill < block_size) hold the KV of `tokens`
  // under the chain `parent`, as a donor of those slots. The caller goes on writing the slots
  // behind them; a later register_block() of the filled block raises the entry to a full one.
  void register_partial(int32_t block, uint64_t parent, const int32_t* tokens, int32_t fill);
  // The donor under `parent` with the longest common head with tokens[0:n), capped at max_j
  // and at the donor's valid slots: returns the block with a reference taken (the caller
  // releases it once the copy is planned) and the head's length in *j, or -1 when no donor
  // shares at least min_j tokens.
  int32_t match_head(uint64_t parent, const int32_t* tokens, int32_t n, int32_t max_j, int32_t min_j,
                     int32_t* j);
  void add_ref(int32_t block);  // one more user of a block that is in use (ref > 0)
  int32_t ref_count(int32_t block) const { return ref_[block]; }
  int32_t num_donors() const { return num_donors_; }
  void reset();
  // ---- host tier
  int32_t host_slots() const { return host_slots_; }
  int32_t num_host_cached() const { return (int32_t)host_dir_.size(); }
  // the device block / host slot holding exactly `tokens` under `hash`, or -1: no reference is
  // taken and no LRU order changes
  int32_t peek(uint64_t hash, const int32_t* tokens) const;
  int32_t host_peek(uint64_t hash, const int32_t* tokens) const;
  // keep `slot` (d = +1) from being evicted while a lookup that found it goes on; d = -1 undoes it
  void host_pin(int32_t slot, int32_t d);
  // Bring the block in `slot` back: a device block is allocated (evicting, and so perhaps
  // spilling, as any allocation), registered under the slot's hash as a reused block with one
  // reference taken, and the fill (slot, block) is listed. -1 when no block can be allocated or
  // the hash is resident on the device already.
  int32_t restore(int32_t slot);
  // the moves planned since the last call, in planning order; unpins their slots
  void take_moves(std::vector<KvMove>& spills, std::vector<KvMove>& fills);
  void reset_host();  // forget every slot that no pending move names
  int64_t host_hit_blocks() const { return host_hits_; }
  int64_t host_spilled_blocks() const { return host_spilled_; }
  int64_t host_evicted_blocks() const { return host_evicted_; }

 private:
  void evict_one();
  void spill(int32_t b);       // evict_one: list the block for the host tier, if it is one to keep
  int32_t take_host_slot();    // a free slot, or the oldest unpinned one (its entry is dropped), or -1
  void host_touch(int32_t slot);
  void donor_add(int32_t b, uint64_t parent, int32_t fill);
  void donor_drop(int32_t b);
  void forget(int32_t b);  // the block leaves the cache: hash entry, donor entry, tokens
  int32_t num_blocks_, block_size_;
  bool prefix_caching_;
  std::vector<int32_t> ref_;
  std::vector<uint64_t> hash_;
  std::vector<char> hashed_;
  std::vector<std::vector<int32_t>> tokens_;  // verification copy for registered blocks
  std::vector<int32_t> free_list_;
  std::unordered_map<uint64_t, int32_t> cache_;
  void lru_remove(int32_t b);
  void lru_push(int32_t b, int list);
  std::list<int32_t> lru_[2];  // evictable (ref == 0, hashed), front = oldest: [0] probation, [1] protected
  std::vector<std::list<int32_t>::iterator> lru_pos_;
  std::vector<char> in_lru_;   // 0 = not evictable, 1 = probation, 2 = protected
  std::vector<char> reused_;   // looked up at least once since it was computed
  // donor index: parent hash -> blocks listed under it; fill_[b] > 0 = b is listed (under
  // dparent_[b]) and tokens_[b][0:fill_[b]) are the tokens of its valid slots
  std::unordered_map<uint64_t, std::vector<int32_t>> donors_;
  std::vector<uint64_t> dparent_;
  std::vector<int32_t> fill_;
  int32_t num_donors_ = 0;
  // host tier: slot -> hash, parent hash and verification tokens of the block it holds
  int32_t host_slots_ = 0;
  std::unordered_map<uint64_t, int32_t> host_dir_;
  std::vector<uint64_t> h_hash_, h_parent_;
  std::vector<std::vector<int32_t>> h_tokens_;
  std::vector<int32_t> h_pin_;      // pending moves and lookups in progress that name the slot
  std::vector<char> h_used_;
  std::vector<int32_t> host_free_;
  std::list<int32_t> host_lru_;     // slots in use, front = oldest
  std::vector<std::list<int32_t>::iterator> host_pos_;
  std::vector<KvMove> spills_, fills_;
  int64_t host_hits_ = 0, host_spilled_ = 0, host_evicted_ = 0;
};

}  // namespace rt
