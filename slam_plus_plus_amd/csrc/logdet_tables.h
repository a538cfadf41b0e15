// logdet_tables.h -- where the scalar pivots of a plan's factor live (slampp_hip_logdet): one entry per scalar row of the
// system, block column by block column in the plan's order.  An entry >= 0 is an offset into the factor's values (d_L): the
// diagonal block is the first block of its column, column-major, so pivot i of a d x d block at loff sits at loff + i (d + 1).
// An entry < 0 stands for a column eliminated inside the dense top: -(1 + p), p = dense_pos + i its position on the diagonal
// of the dense matrix (element p (ld + 1) with ld the padded dimension, which the plan does not know).  Padding and
// alignment gaps of the dense top carry identity and have no entry.  Plans over block columns that were cut into pieces
// need nothing special: the scalar factor is the same.
// Depends on plan.h only, no device calls: compiled on its own under the sanitizers (tests/logdet_tables_driver.cpp).
#pragma once
#include "plan.h"

namespace slampp {

void build_logdet_table(const Plan &plan, std::vector<int64_t> &r_table);

} // namespace slampp
