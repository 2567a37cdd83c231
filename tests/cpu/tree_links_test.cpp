// tree_links_test.cpp -- mpboot_amd/host/tree_links.hpp without a GPU, under the address and undefined-behaviour sanitizers:
// the layout of random topologies against a plain restatement of the two loops it replaced, and the corruptions it must reject.
//   tree_links_test layout <seed> <trees>      tree_links_test reject <seed> <trees>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../mpboot_amd/host/tree_links.hpp"

struct Pair { uint32_t x, y; };

static void hookup(std::vector<int32_t> &back, int a, int b) { back[a] = b; back[b] = a; }

// a random topology by stepwise addition: exactly 3 (2n - 1) entries (the sanitizer sees every read past them); record 3v of tip v,
// 3v .. 3v + 2 of inner node v, everything else -1
static std::vector<int32_t> random_tree(int n, std::mt19937 &rng)
{
  std::vector<int32_t> back(3 * (size_t)(2 * n - 1), -1);
  int next_inner = n + 1;
  const int c = next_inner++;
  for (int s = 0; s < 3; s++) hookup(back, 3 * c + s, 3 * (s + 1));
  std::vector<int> branches = {3, 6, 9};          // one record per branch
  for (int t = 4; t <= n; t++) {
    const int r = branches[rng() % branches.size()], q = back[r];
    const int v = next_inner++;
    const int rot = (int)(rng() % 3);              // which of the new node's records takes which neighbour
    const int a = 3 * v + rot, b = 3 * v + (rot + 1) % 3, d = 3 * v + (rot + 2) % 3;
    hookup(back, a, r);
    hookup(back, b, q);
    hookup(back, d, 3 * t);
    branches.push_back(b);
    branches.push_back(3 * t);
  }
  return back;
}

// the separate loops, as they stood in Engine::set_tree and Engine::schedule_views_dev
static uint32_t slot(int r, int n) { const int v = r / 3; return v <= n ? (uint32_t)(v - 1) : (uint32_t)(n + 3 * (v - n - 1) + r % 3); }
static bool plain_check(int n, const std::vector<int32_t> &back)
{
  const size_t len = 3 * (size_t)(2 * n - 1);
  for (int v = 1; v <= 2 * n - 2; v++)
    for (int s = 0; s < (v <= n ? 1 : 3); s++) {
      const int r = 3 * v + s, b = back[r];
      if (b < 3 || b >= (int)len || back[b] != r) return false;
    }
  return true;
}
static void plain_layout(int n, const std::vector<int32_t> &back, std::vector<Pair> &kids)
{
  for (int v = n + 1; v <= 2 * n - 2; v++) {
    const int r0 = 3 * v;
    const uint32_t s0 = slot(back[r0], n), s1 = slot(back[r0 + 1], n), s2 = slot(back[r0 + 2], n);
    Pair *k = &kids[slot(r0, n)];
    k[0] = Pair{s1, s2};
    k[1] = Pair{s2, s0};
    k[2] = Pair{s0, s1};
  }
}

static int run_layout(unsigned seed, int trees)
{
  std::mt19937 rng(seed);
  for (int t = 0; t < trees; t++) {
    const int n = 4 + (int)(rng() % 197);          // 4 .. 200 taxa
    const std::vector<int32_t> back = random_tree(n, rng);
    const size_t ns = (size_t)n + 3 * (size_t)(n - 2);
    std::vector<Pair> want(ns, Pair{0xABCDu, 0xABCDu}), got(ns, Pair{0xABCDu, 0xABCDu});   // exactly the slots: a write past them is seen
    if (!plain_check(n, back)) { std::printf("tree %d: the generator's tree fails the plain check\n", t); return 1; }
    plain_layout(n, back, want);
    if (!mpf::links::check_and_layout(n, back.data(), got.data())) { std::printf("tree %d (n = %d): rejected\n", t, n); return 1; }
    if (!mpf::links::check_and_layout<Pair>(n, back.data(), nullptr)) { std::printf("tree %d (n = %d): rejected by the check alone\n", t, n); return 1; }
    std::vector<Pair> alone(ns, Pair{0xABCDu, 0xABCDu});                                   // the layout without the check
    (void)mpf::links::check_and_layout<Pair, false>(n, back.data(), alone.data());
    for (size_t i = 0; i < ns; i++)
      if (want[i].x != got[i].x || want[i].y != got[i].y || want[i].x != alone[i].x || want[i].y != alone[i].y) { std::printf("tree %d (n = %d): DIFFERENT at slot %zu\n", t, n, i); return 1; }
  }
  std::printf("%d layouts equal\n", trees);
  return 0;
}

static int run_reject(unsigned seed, int trees)
{
  std::mt19937 rng(seed);
  int rejected[4] = {0, 0, 0, 0};
  for (int t = 0; t < trees; t++) {
    const int n = 4 + (int)(rng() % 197);
    const std::vector<int32_t> good = random_tree(n, rng);
    const int len = 3 * (2 * n - 1);
    const size_t ns = (size_t)n + 3 * (size_t)(n - 2);
    // a record in use: a tip's first or any of an inner node's
    const int v = 1 + (int)(rng() % (2 * n - 2));
    const int r = 3 * v + (v <= n ? 0 : (int)(rng() % 3));
    for (int kind = 0; kind < 4; kind++) {
      std::vector<int32_t> bad = good;
      if (kind == 0) bad[r] = (int)(rng() % 5) - 2;                    // a link below 3 (-2 .. 2)
      else if (kind == 1) bad[r] = len + (int)(rng() % 3);             // a link at or past the end
      else if (kind == 2) {                                            // a one-way link: r points at a record that points elsewhere
        int other;
        do { const int u = 1 + (int)(rng() % (2 * n - 2)); other = 3 * u + (u <= n ? 0 : (int)(rng() % 3)); } while (other == good[r] || other == r);
        bad[r] = other;
      } else bad[r] = 3 * (1 + (int)(rng() % n)) + 1 + (int)(rng() % 2);   // a link into a tip's unused record
      std::vector<Pair> kids(ns);
      const bool plain = plain_check(n, bad);
      const bool ours = mpf::links::check_and_layout(n, bad.data(), kids.data());
      const bool alone = mpf::links::check_and_layout<Pair>(n, bad.data(), nullptr);
      if (plain || ours || alone) { std::printf("tree %d (n = %d) kind %d: ACCEPTED (plain %d, layout %d, check %d)\n", t, n, kind, plain, ours, alone); return 1; }
      rejected[kind]++;
    }
  }
  std::printf("rejected: below-3 %d, past-the-end %d, one-way %d, tip-unused %d\n", rejected[0], rejected[1], rejected[2], rejected[3]);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc < 4) { std::fprintf(stderr, "usage: tree_links_test layout|reject <seed> <trees>\n"); return 2; }
  const unsigned seed = (unsigned)std::atoi(argv[2]);
  const int trees = std::atoi(argv[3]);
  if (argv[1][0] == 'l') return run_layout(seed, trees);
  if (argv[1][0] == 'r') return run_reject(seed, trees);
  return 2;
}
