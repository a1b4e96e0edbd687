// Batch-unique gather/scatter lists on the host (unique_lists.h).
#include "unique_lists.h"

#include <algorithm>

namespace wf {

int UniqueLists::largest() const
{
  int most = 0;
  for (size_t b = 0; b + 1 < uoff.size(); ++b) most = std::max(most, uoff[b + 1] - uoff[b]);
  return most;
}

bool build_unique_lists(const int32_t* dofmap, size_t ncells, int nd, int CB, UniqueLists* out)
{
  const size_t nbatch = (ncells + CB - 1) / CB;
  out->uoff.assign(nbatch + 1, 0);
  out->uniq.clear();
  out->uniq.reserve(ncells * nd / 2);
  out->loc.resize(ncells * nd);
  std::vector<int32_t> tmp;
  for (size_t b = 0; b < nbatch; ++b) {
    const size_t c0 = b * CB, nc = std::min<size_t>(CB, ncells - c0);
    tmp.assign(dofmap + c0 * nd, dofmap + (c0 + nc) * nd);
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    if (tmp.size() > 65535) return false;
    for (size_t e = c0 * nd; e < (c0 + nc) * nd; ++e)
      out->loc[e] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), dofmap[e]) - tmp.begin());
    out->uniq.insert(out->uniq.end(), tmp.begin(), tmp.end());
    out->uoff[b + 1] = (int32_t)out->uniq.size();
  }
  return true;
}

std::vector<uint32_t> pack_dense_loc(const std::vector<uint16_t>& loc, size_t ncells, int nd, int KT, int NCB)
{
  const size_t nbatch = (ncells + NCB - 1) / NCB, KT2 = (size_t)(KT + 1) / 2;
  std::vector<uint32_t> locP(nbatch * KT2 * 4 * NCB, 0);
  for (size_t cell = 0; cell < ncells; ++cell)
    for (int k = 0; k < nd; ++k) {
      const size_t b = cell / NCB, c = cell % NCB, ks = (size_t)k / 4, lg = (size_t)k % 4;
      locP[((b * KT2 + ks / 2) * 4 + lg) * NCB + c] |= (uint32_t)loc[cell * nd + k] << (16 * (ks & 1));
    }
  return locP;
}

}  // namespace wf
