// logdet_tables.cpp -- the pivot table of slampp_hip_logdet (logdet_tables.h), host only
#include "logdet_tables.h"

namespace slampp {

void build_logdet_table(const Plan &plan, std::vector<int64_t> &r_table)
{
	const Plan &P = plan;
	r_table.clear();
	r_table.reserve(P.cs_new.empty()? 0 : size_t(P.cs_new[size_t(P.n)]));
	for(int32_t j = 0; j < P.n; ++ j) {
		const int d = P.dim[size_t(j)];
		if(P.dense_dim && P.dense_pos[size_t(j)] >= 0) {
			for(int i = 0; i < d; ++ i)
				r_table.push_back(-(int64_t(1) + P.dense_pos[size_t(j)] + i));
		} else {
			const int64_t n_loff = P.loff[size_t(P.lptr[size_t(j)])];
			for(int i = 0; i < d; ++ i)
				r_table.push_back(n_loff + int64_t(i) * (d + 1));
		}
	}
}

} // namespace slampp
