// Host-only driver of csrc/tail_queue.h (tests/test_tail_queue_cpu.py): the plan, the static walks and the ticket rules are the
// functions the kernels call, executed here on the CPU.  Built with `hipcc --offload-host-only`; needs no GPU.
// One command per line of stdin (key=value tokens):
//   plan T= tail=                  -> "S tail grid" of o2_tail_plan
//   arg T= tail_arg= rounds= slots= -> "S tail grid" of o2_tail_plan_arg (what the entry points do with their `tail` argument)
//   sim walk=round|range T= tail= [ends=e1,e2,...] tickets=t0,t1,...
//       a launch of the plan (T, tail): workgroup b < S walks statically, workgroup S + i draws ticket t_i.  Prints the plan, then
//       "tiles:" with the tile of every workgroup of the grid (-1: the workgroup returns; with ends= the tile as problem:local tile
//       of a grouped launch whose problems end at e1, e2, ...), then "resets:" with the workgroups that zero the counter.
#include <hip/hip_runtime.h>
#include "tail_queue.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace {
typedef std::map<std::string, std::string> KV;
long long geti(const KV& kv, const char* k, long long dflt) {
  auto it = kv.find(k);
  return it == kv.end() ? dflt : strtoll(it->second.c_str(), nullptr, 0);
}
std::vector<long long> getlist(const KV& kv, const char* k) {
  std::vector<long long> v;
  auto it = kv.find(k);
  if (it == kv.end()) return v;
  std::istringstream in(it->second);
  std::string tok;
  while (std::getline(in, tok, ',')) v.push_back(strtoll(tok.c_str(), nullptr, 0));
  return v;
}
struct Prob { int tile_end; };
struct Group { int n; Prob p[16]; };
}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    if (!(in >> cmd) || cmd[0] == '#') continue;
    KV kv;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq != std::string::npos) kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    if (cmd == "plan" || cmd == "arg" || cmd == "sim") {
      const O2TailPlan p = cmd == "arg" ? o2_tail_plan_arg(geti(kv, "T", 0), (int)geti(kv, "tail_arg", 0), (int)geti(kv, "rounds", 0),
                                                           (int)geti(kv, "slots", 0))
                                        : o2_tail_plan(geti(kv, "T", 0), geti(kv, "tail", 0));
      printf("%d %d %d\n", p.S, p.tail, p.grid);
      if (cmd != "sim") continue;
      const bool round = kv["walk"] == "round";
      const std::vector<long long> tickets = getlist(kv, "tickets"), ends = getlist(kv, "ends");
      if ((long long)tickets.size() != (long long)p.grid - p.S || ends.size() > 16) {
        fprintf(stderr, "sim: %zu tickets for %d workgroups past S\n", tickets.size(), p.grid - p.S);
        return 2;
      }
      Group g;
      g.n = (int)ends.size();
      for (int i = 0; i < g.n; ++i) g.p[i].tile_end = (int)ends[i];
      std::string resets;
      printf("tiles:");
      for (int b = 0; b < p.grid; ++b) {
        int id;
        if (b < p.S) id = round ? o2_xcd_round_id(b, p.S) : o2_xcd_range_id(b, p.S);
        else {
          const unsigned int t = (unsigned int)tickets[b - p.S];
          id = o2_tail_ticket_tile(p.S, p.tail, t);
          if (o2_tail_ticket_resets(p.tail, t)) resets += " " + std::to_string(b);
        }
        if (g.n && id >= 0) {
          int first;
          const int pi = o2_group_problem(g, id, first);
          printf(" %d:%d", pi, id - first);
        } else printf(" %d", id);
      }
      printf("\nresets:%s\n", resets.c_str());
    } else {
      fprintf(stderr, "unknown command: %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
