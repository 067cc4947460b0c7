#include "block_manager.h"

#include <algorithm>
#include <cstring>

namespace rt {

uint64_t hash_block(uint64_t parent, const int32_t* tokens, int n) {
  uint64_t h = parent ^ 0x9E3779B97F4A7C15ULL;
  for (int i = 0; i < n; ++i) {
    uint64_t x = (uint64_t)(uint32_t)tokens[i] + 0x632BE59BD9B4E019ULL * (uint64_t)(i + 1);
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    h = (h ^ x) * 0x100000001B3ULL + 0x7F4A7C159E3779B9ULL;
  }
  h ^= h >> 29;
  h *= 0xc4ceb9fe1a85ec53ULL;
  h ^= h >> 32;
  return h ? h : 1;
}

BlockManager::BlockManager(int32_t num_blocks, int32_t block_size, bool prefix_caching, int32_t host_slots)
    : num_blocks_(num_blocks), block_size_(block_size), prefix_caching_(prefix_caching),
      host_slots_(prefix_caching ? std::max(0, host_slots) : 0) {
  reset();
}

void BlockManager::reset() {
  ref_.assign(num_blocks_, 0);
  hash_.assign(num_blocks_, 0);
  hashed_.assign(num_blocks_, 0);
  tokens_.assign(num_blocks_, {});
  lru_[0].clear();
  lru_[1].clear();
  lru_pos_.assign(num_blocks_, lru_[0].end());
  in_lru_.assign(num_blocks_, 0);
  reused_.assign(num_blocks_, 0);
  donors_.clear();
  dparent_.assign(num_blocks_, 0);
  fill_.assign(num_blocks_, 0);
  num_donors_ = 0;
  cache_.clear();
  free_list_.clear();
  free_list_.reserve(num_blocks_);
  for (int32_t b = num_blocks_ - 1; b >= 0; --b) free_list_.push_back(b);
  // the host tier goes with the cache it extends; moves not taken yet name blocks that no
  // longer mean anything
  spills_.clear();
  fills_.clear();
  h_pin_.assign(host_slots_, 0);
  reset_host();
}

void BlockManager::reset_host() {
  if (host_slots_ <= 0) return;
  h_hash_.resize(host_slots_, 0);
  h_parent_.resize(host_slots_, 0);
  h_tokens_.resize(host_slots_);
  h_used_.resize(host_slots_, 0);
  host_pos_.resize(host_slots_, host_lru_.end());
  for (int32_t s = 0; s < host_slots_; ++s) {
    if (!h_used_[s] || h_pin_[s] > 0) continue;
    host_dir_.erase(h_hash_[s]);
    host_lru_.erase(host_pos_[s]);
    h_used_[s] = 0;
    h_tokens_[s].clear();
  }
  host_free_.clear();
  for (int32_t s = host_slots_ - 1; s >= 0; --s)
    if (!h_used_[s]) host_free_.push_back(s);
}

void BlockManager::host_touch(int32_t slot) {
  host_lru_.erase(host_pos_[slot]);
  host_lru_.push_back(slot);
  host_pos_[slot] = std::prev(host_lru_.end());
}

int32_t BlockManager::take_host_slot() {
  if (!host_free_.empty()) {
    const int32_t s = host_free_.back();
    host_free_.pop_back();
    return s;
  }
  for (const int32_t s : host_lru_) {
    if (h_pin_[s] > 0) continue;
    host_dir_.erase(h_hash_[s]);
    host_lru_.erase(host_pos_[s]);
    h_used_[s] = 0;
    ++host_evicted_;
    return s;
  }
  return -1;
}

void BlockManager::spill(int32_t b) {
  if (host_slots_ <= 0 || !hashed_[b] || (int32_t)tokens_[b].size() != block_size_) return;
  auto it = host_dir_.find(hash_[b]);
  if (it != host_dir_.end()) {  // inclusive tier: the slot already holds these bytes
    if (h_tokens_[it->second] == tokens_[b]) host_touch(it->second);
    return;
  }
  const int32_t s = take_host_slot();
  if (s < 0) return;  // every slot is pinned: dropped, as without the tier
  h_hash_[s] = hash_[b];
  h_parent_[s] = dparent_[b];
  h_tokens_[s] = tokens_[b];
  h_used_[s] = 1;
  host_lru_.push_back(s);
  host_pos_[s] = std::prev(host_lru_.end());
  host_dir_.emplace(hash_[b], s);
  ++h_pin_[s];
  spills_.push_back({b, s});
  ++host_spilled_;
}

int32_t BlockManager::peek(uint64_t hash, const int32_t* tokens) const {
  if (!prefix_caching_) return -1;
  auto it = cache_.find(hash);
  if (it == cache_.end()) return -1;
  const int32_t b = it->second;
  if ((int32_t)tokens_[b].size() != block_size_ ||
      std::memcmp(tokens_[b].data(), tokens, sizeof(int32_t) * block_size_) != 0)
    return -1;
  return b;
}

int32_t BlockManager::host_peek(uint64_t hash, const int32_t* tokens) const {
  if (host_slots_ <= 0) return -1;
  auto it = host_dir_.find(hash);
  if (it == host_dir_.end()) return -1;
  const int32_t s = it->second;
  if ((int32_t)h_tokens_[s].size() != block_size_ ||
      std::memcmp(h_tokens_[s].data(), tokens, sizeof(int32_t) * block_size_) != 0)
    return -1;
  return s;
}

void BlockManager::host_pin(int32_t slot, int32_t d) {
  if (slot < 0 || slot >= host_slots_) return;
  h_pin_[slot] = std::max(0, h_pin_[slot] + d);
}

int32_t BlockManager::restore(int32_t slot) {
  if (slot < 0 || slot >= host_slots_ || !h_used_[slot]) return -1;
  if (cache_.count(h_hash_[slot])) return -1;
  ++h_pin_[slot];  // the allocation below may evict into the tier: not into this slot
  std::vector<int32_t> out;
  if (!allocate(1, out)) {
    --h_pin_[slot];
    return -1;
  }
  const int32_t b = out[0];
  register_block(b, h_hash_[slot], h_tokens_[slot].data(), h_parent_[slot]);
  reused_[b] = 1;
  host_touch(slot);
  fills_.push_back({b, slot});  // the pin stays until the move is taken
  ++host_hits_;
  return b;
}

void BlockManager::take_moves(std::vector<KvMove>& spills, std::vector<KvMove>& fills) {
  for (const KvMove& m : spills_) host_pin(m.slot, -1);
  for (const KvMove& m : fills_) host_pin(m.slot, -1);
  spills.swap(spills_);
  fills.swap(fills_);
  spills_.clear();
  fills_.clear();
}

void BlockManager::lru_remove(int32_t b) {
  if (!in_lru_[b]) return;
  lru_[in_lru_[b] - 1].erase(lru_pos_[b]);
  in_lru_[b] = 0;
}

void BlockManager::lru_push(int32_t b, int list) {
  lru_[list].push_back(b);
  lru_pos_[b] = std::prev(lru_[list].end());
  in_lru_[b] = (char)(list + 1);
}

void BlockManager::donor_add(int32_t b, uint64_t parent, int32_t fill) {
  if (fill_[b] > 0) {  // already listed (a partial tail that filled up): same parent, more slots
    fill_[b] = fill;
    return;
  }
  donors_[parent].push_back(b);
  dparent_[b] = parent;
  fill_[b] = fill;
  ++num_donors_;
}

void BlockManager::donor_drop(int32_t b) {
  if (fill_[b] <= 0) return;
  auto it = donors_.find(dparent_[b]);
  if (it != donors_.end()) {
    std::vector<int32_t>& v = it->second;
    auto p = std::find(v.begin(), v.end(), b);
    if (p != v.end()) {
      *p = v.back();
      v.pop_back();
    }
    if (v.empty()) donors_.erase(it);
  }
  fill_[b] = 0;
  --num_donors_;
}

void BlockManager::forget(int32_t b) {
  if (hashed_[b]) {
    auto it = cache_.find(hash_[b]);
    if (it != cache_.end() && it->second == b) cache_.erase(it);
  }
  donor_drop(b);
  hashed_[b] = 0;
  reused_[b] = 0;
  tokens_[b].clear();
}

void BlockManager::evict_one() {
  const int list = lru_[0].empty() ? 1 : 0;  // never-reused blocks first
  const int32_t b = lru_[list].front();
  lru_remove(b);
  spill(b);
  forget(b);
  free_list_.push_back(b);
}

bool BlockManager::allocate(int32_t n, std::vector<int32_t>& out) {
  if (n <= 0) return true;
  if (num_free() < n) return false;
  for (int32_t i = 0; i < n; ++i) {
    if (free_list_.empty()) evict_one();
    const int32_t b = free_list_.back();
    free_list_.pop_back();
    ref_[b] = 1;
    out.push_back(b);
  }
  return true;
}

void BlockManager::release(int32_t b) {
  if (b < 0 || b >= num_blocks_ || ref_[b] <= 0) return;
  if (--ref_[b] > 0) return;
  if ((hashed_[b] || fill_[b] > 0) && prefix_caching_) {
    if (reused_[b]) {
      lru_push(b, 1);
      if ((int32_t)lru_[1].size() > num_blocks_ / 2) {  // protected segment full: demote its oldest
        const int32_t d = lru_[1].front();
        lru_remove(d);
        lru_push(d, 0);
      }
    } else {
      lru_push(b, 0);
    }
  } else {
    forget(b);
    free_list_.push_back(b);
  }
}

void BlockManager::add_ref(int32_t b) {
  if (b < 0 || b >= num_blocks_ || ref_[b] <= 0) return;
  ++ref_[b];
}

int32_t BlockManager::lookup(uint64_t hash, const int32_t* tokens) {
  if (!prefix_caching_) return -1;
  auto it = cache_.find(hash);
  if (it == cache_.end()) return -1;
  const int32_t b = it->second;
  if ((int32_t)tokens_[b].size() != block_size_ ||
      std::memcmp(tokens_[b].data(), tokens, sizeof(int32_t) * block_size_) != 0)
    return -1;
  lru_remove(b);
  reused_[b] = 1;
  ++ref_[b];
  return b;
}

void BlockManager::register_block(int32_t b, uint64_t hash, const int32_t* tokens, uint64_t parent) {
  if (!prefix_caching_ || hashed_[b]) return;
  auto it = cache_.find(hash);
  if (it != cache_.end()) return;  // an identical page is already cached; keep this one private
  cache_.emplace(hash, b);
  hash_[b] = hash;
  hashed_[b] = 1;
  tokens_[b].assign(tokens, tokens + block_size_);
  donor_add(b, parent, block_size_);
}

void BlockManager::register_partial(int32_t b, uint64_t parent, const int32_t* tokens, int32_t fill) {
  if (!prefix_caching_ || b < 0 || b >= num_blocks_ || ref_[b] <= 0) return;
  if (fill <= 0 || fill >= block_size_ || hashed_[b] || fill_[b] > 0) return;
  tokens_[b].assign(tokens, tokens + fill);
  donor_add(b, parent, fill);
}

int32_t BlockManager::match_head(uint64_t parent, const int32_t* tokens, int32_t n, int32_t max_j,
                                 int32_t min_j, int32_t* j) {
  *j = 0;
  if (!prefix_caching_) return -1;
  auto it = donors_.find(parent);
  if (it == donors_.end()) return -1;
  const int32_t cap = std::min(std::min(n, max_j), block_size_);
  int32_t best = -1, best_j = 0;
  for (const int32_t d : it->second) {
    const int32_t m = std::min<int32_t>(cap, std::min<int32_t>(fill_[d], (int32_t)tokens_[d].size()));
    int32_t c = 0;
    while (c < m && tokens_[d][c] == tokens[c]) ++c;
    if (c > best_j) {
      best_j = c;
      best = d;
      if (c == cap) break;
    }
  }
  if (best < 0 || best_j < std::max(1, min_j)) return -1;
  lru_remove(best);
  reused_[best] = 1;
  ++ref_[best];
  *j = best_j;
  return best;
}

}  // namespace rt
