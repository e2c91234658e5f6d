// The witness check's share of a proving key (check.hip); the key itself is PkDev (prover.h).
#pragma once

#include <memory>
#include <mutex>
#include <vector>

#include "poly.h"

namespace zg {

// Per proving key, built at the FIRST check (zg_prover_create costs what it cost before) and shared read-only by
// every prover forked from the key: the permutation mapping recovered from the sigma values and the sorted tuples
// of the lookup tables that read fixed columns only.  Defined in check.hip; freed with the key.
struct CheckKey;

// The host's copy of the few circuit facts the check decides by (filled by zg_prover_create), the lock the key data
// is built under, and the key data.
struct CheckInfo {
    std::vector<zg_query> perm_cols;
    std::vector<uint32_t> lookup_width;
    std::vector<uint8_t> table_var;  // 1: a table polynomial of this lookup queries an advice or instance cell
    std::mutex mu;
    std::shared_ptr<CheckKey> key;
};

}  // namespace zg
