// TEST INFRASTRUCTURE (tests/test_oracle_draw_cpu.py): the real std::discrete_distribution<int> over a std::mt19937 whose
// next outputs are given words -- what oracle/linearham_oracle.discrete_distribution_draw restates.
//
// stdin, one draw per line:   <word0> <word1> <n> <weight 0> ... <weight n-1>     (weights as C99 hex floats, inf, nan)
// stdout, one line per draw:  <index drawn> <engine outputs consumed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

// the state word whose tempered value is y (inverse of std::mt19937's output transformation)
static uint32_t Untemper(uint32_t y) {
  y ^= y >> 18;
  y ^= (y << 15) & 0xEFC60000u;
  uint32_t t = y;
  for (int i = 0; i < 5; ++i) t = y ^ ((t << 7) & 0x9D2C5680u);
  y = t;
  for (int i = 0; i < 3; ++i) t = y ^ (t >> 11);
  return t;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    uint32_t w0, w1;
    size_t n;
    if (!(in >> w0 >> w1 >> n)) continue;
    std::vector<double> weights(n);
    std::string tok;
    for (size_t i = 0; i < n; ++i) {
      in >> tok;
      weights[i] = std::strtod(tok.c_str(), nullptr);
    }
    // the engine's text form is its 624 state words and the position of the next one: outputs w0, w1, then 2, 3, ...
    std::ostringstream st;
    for (uint32_t i = 0; i < 624; ++i) st << Untemper(i == 0 ? w0 : i == 1 ? w1 : i) << ' ';
    st << 0;
    std::istringstream state(st.str());
    std::mt19937 rng;
    state >> rng;
    const std::mt19937 before = rng;
    std::discrete_distribution<int> dist(weights.begin(), weights.end());
    const int k = dist(rng);
    int used = -1;
    for (int c = 0; c <= 8 && used < 0; ++c) {
      std::mt19937 probe = before;
      probe.discard(c);
      if (probe == rng) used = c;
    }
    std::printf("%d %d\n", k, used);
  }
  return 0;
}
