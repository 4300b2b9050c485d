// Host build of the snapshot validation and merge (banjax_amd/csrc/snapshot.h)
// for tests/test_state_snapshot_cpu.py: as a shared library through ctypes, and
// with -DBJX_SNAPSHOT_MAIN as a stand-alone program that runs a corpus file
// (the sanitizer run).
#include <stdio.h>

#include "../../banjax_amd/csrc/snapshot.h"

// 0: a canonical snapshot; 1: rejected, msg names the failed check
extern "C" int bjx_test_snap_validate(const uint8_t *p, uint64_t len, char *msg, uint64_t cap) {
  bjx_snap::Layout L;
  std::vector<std::string> names;
  const char *why = bjx_snap::validate_host(p, len, &L, &names);
  if (!why) why = bjx_snap::check_body(p, L);
  if (msg && cap) snprintf(msg, (size_t)cap, "%s", why ? why : "");
  return why ? 1 : 0;
}

// merged snapshot of n shards into out (cap bytes); 0 ok, 1 rejected, 2 cap too small (*out_len set)
extern "C" int bjx_test_snap_merge(uint32_t n, const uint8_t *const *ptrs, const uint64_t *lens, uint8_t *out, uint64_t cap,
                                   uint64_t *out_len, char *msg, uint64_t msg_cap) {
  std::vector<std::pair<const uint8_t *, uint64_t>> shards;
  for (uint32_t k = 0; k < n; ++k) shards.push_back({ptrs[k], lens[k]});
  std::vector<uint8_t> merged;
  bool capacity = false;
  const char *why = bjx_snap::merge(shards, &merged, &capacity);
  if (msg && msg_cap) snprintf(msg, (size_t)msg_cap, "%s", why ? why : "");
  if (why) return 1;
  *out_len = merged.size();
  if (merged.size() > cap) return 2;
  memcpy(out, merged.data(), merged.size());
  return 0;
}

#ifdef BJX_SNAPSHOT_MAIN
// corpus: cases of {u32 accept, u32 keyword length, keyword, u64 blob length,
// blob}; a rejected blob's message must contain the keyword.  After the cases
// every accepted blob is merged with itself.  Exit 0 when every case came out
// as the corpus says.
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
  fclose(f);
  size_t at = 0, bad = 0, n = 0;
  while (at + 8 <= all.size()) {
    const uint32_t accept = bjx_snap::rd32(&all[at]), kl = bjx_snap::rd32(&all[at + 4]);
    at += 8;
    if (at + kl + 8 > all.size()) return 2;
    const std::string kw(reinterpret_cast<const char *>(&all[at]), kl);
    at += kl;
    const uint64_t bl = bjx_snap::rd64(&all[at]);
    at += 8;
    if (bl > all.size() - at) return 2;
    // an exact-size copy: a read past the blob's end is a read past the allocation
    std::vector<uint8_t> blob(all.begin() + at, all.begin() + at + bl);
    at += bl;
    char msg[256];
    const int rc = bjx_test_snap_validate(blob.data(), blob.size(), msg, sizeof msg);
    const bool ok = accept ? rc == 0 : rc == 1 && strstr(msg, kw.c_str()) != nullptr;
    if (!ok) {
      fprintf(stderr, "case %zu: accept %u, got %d \"%s\" (keyword \"%s\")\n", n, accept, rc, msg, kw.c_str());
      ++bad;
    }
    if (accept && rc == 0) {
      const uint8_t *ptrs[2] = {blob.data(), blob.data()};
      const uint64_t lens[2] = {blob.size(), blob.size()};
      std::vector<uint8_t> out(2 * blob.size());
      uint64_t got = 0;
      if (bjx_test_snap_merge(2, ptrs, lens, out.data(), out.size(), &got, msg, sizeof msg) != 0) ++bad;
    }
    ++n;
  }
  printf("%zu cases, %zu wrong\n", n, bad);
  return bad ? 1 : 0;
}
#endif
