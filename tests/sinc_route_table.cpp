// Driver of tests/test_sinc_route_cpu.py: prints what csrc/sinc_route.h answers for rows of integers read from stdin.
//   S NT allowed 1 <item>          -> sinc_route of the item
//   B NT allowed n <item> x n      -> sinc_batch_route of the n items
//   <item> = len_out len_in sig0 sig1 sig_stride out0 out1 out_stride   (pointers as integers: nothing is dereferenced)
#include <stdio.h>
#include <vector>
#include "sinc_route.h"

static const char* name(par::SincRoute r) {
  switch (r) {
    case par::SincRoute::Block: return "Block";
    case par::SincRoute::StreamMono: return "StreamMono";
    case par::SincRoute::StreamPick: return "StreamPick";
    case par::SincRoute::StreamStereo: return "StreamStereo";
  }
  return "?";
}

int main() {
  char kind;
  int NT, allowed, n;
  while (scanf(" %c %d %d %d", &kind, &NT, &allowed, &n) == 4) {
    std::vector<par_fused_item> items(n > 0 ? n : 0);
    for (auto& f : items) {
      long long len_out, len_in, sig0, sig1, sig_stride, out0, out1, out_stride;
      if (scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &len_out, &len_in, &sig0, &sig1, &sig_stride, &out0, &out1, &out_stride) != 8) return 2;
      f = par_fused_item{nullptr, 2, nullptr, nullptr, len_out, len_out, reinterpret_cast<const float*>(sig0),
                         reinterpret_cast<const float*>(sig1), sig_stride, len_in, reinterpret_cast<float*>(out0),
                         reinterpret_cast<float*>(out1), out_stride};
    }
    if (kind == 'S' && n != 1) return 2;
    puts(name(kind == 'S' ? par::sinc_route(items[0], NT, allowed != 0) : par::sinc_batch_route(n, items.data(), NT, allowed != 0)));
  }
  return 0;
}
