// simt_device.inl -- what the lane-per-task kernels share (simt_kernel.hip, simt_factor_ahead.hip).  First a lane's loads and
// stores of its own D x D blocks, the reciprocal square root and the walk through a shape's program; then the operand of a
// written-out wait, the timing record's prologue and the occupancy query; then the column arithmetic itself: every sum of the
// factor kernels and of the backward kernels is written once, here, and the forms of a kernel (fetch by column, fetch ahead,
// branches) call it.  That the forms store the same bits -- the tests compare them with array_equal -- follows from that, not
// from copies kept alike by hand.  (Two nests are also written out in a kernel, each marked at its helper below: the product with
// inv(L_jj)^T for odd D in factor_simt_kernel, the solve with L_jj^T in bwd_ahead_solve; profiles/simt_shared_arith_isa.txt.)  A form owns what makes it a form: where a column's operands come from and when (touches,
// register sets, pins, written-out waits), who stores the diagonal block, where the clock samples are taken.
// Expressions and loop orders here are fixed: no sum is reassociated, a -= b * c stays a -= b * c.
// Included inside namespace slampp.

__device__ __forceinline__ double simt_rsqrt(double x)
{
	double y = __builtin_amdgcn_rsq(x);
	const double h = 0.5 * x;
	y = y * (1.5 - h * y * y);
	y = y * (1.5 - h * y * y);
	return y;
}

// D consecutive doubles at p (16-byte aligned when D is even: block offsets are multiples of D * D)
template <int D>
__device__ __forceinline__ void load_column(const double *__restrict__ p, double (&v)[D])
{
	if(D % 2 == 0) {
		const double2 *p2 = reinterpret_cast<const double2*>(p);
		#pragma unroll
		for(int i = 0; i < D / 2; ++ i) {
			const double2 t = p2[i];
			v[2 * i] = t.x;
			v[2 * i + 1] = t.y;
		}
	} else {
		#pragma unroll
		for(int i = 0; i < D; ++ i)
			v[i] = p[i];
	}
}

template <int D>
__device__ __forceinline__ void load_block(const double *__restrict__ p, double (&v)[D][D]) // v[c][r] = p[r + c D]
{
	if(D % 2 == 0) {
		const double2 *p2 = reinterpret_cast<const double2*>(p);
		#pragma unroll
		for(int i = 0; i < D * D / 2; ++ i) {
			const double2 t = p2[i];
			v[(2 * i) / D][(2 * i) % D] = t.x;
			v[(2 * i + 1) / D][(2 * i + 1) % D] = t.y;
		}
	} else {
		#pragma unroll
		for(int i = 0; i < D * D; ++ i)
			v[i / D][i % D] = p[i];
	}
}

// the lower triangle of a block: v[q][r] = p[r + q D] for r >= q (even D: 16-byte loads; the element above the diagonal that
// shares one with the diagonal element of an odd column comes along)
template <int D>
__device__ __forceinline__ void load_lower(const double *__restrict__ p, double (&v)[D][D])
{
	#pragma unroll
	for(int q = 0; q < D; ++ q) {
		if(D % 2 == 0) {
			#pragma unroll
			for(int r = q & ~1; r < D; r += 2) {
				const double2 t = *reinterpret_cast<const double2*>(p + r + q * D);
				v[q][r] = t.x;
				v[q][r + 1] = t.y;
			}
		} else {
			#pragma unroll
			for(int r = q; r < D; ++ r)
				v[q][r] = p[r + q * D];
		}
	}
}

template <int D>
__device__ __forceinline__ void store_block(double *p, const double (&m)[D][D]) // m[r][q] -> p[r + q D]
{
	if(D % 2 == 0) {
		double2 *p2 = reinterpret_cast<double2*>(p);
		#pragma unroll
		for(int q = 0; q < D; ++ q) {
			#pragma unroll
			for(int r = 0; r < D; r += 2)
				p2[(r + q * D) / 2] = double2{m[r][q], m[r + 1][q]};
		}
	} else {
		#pragma unroll
		for(int q = 0; q < D; ++ q) {
			#pragma unroll
			for(int r = 0; r < D; ++ r)
				p[r + q * D] = m[r][q];
		}
	}
}

// rows [r0, r0 + D / 2) of a block: v[c][i] = p[r0 + i + c D] (two lanes per task: each takes half the rows)
template <int D>
__device__ __forceinline__ void load_half_rows(const double *__restrict__ p, int r0, double (&v)[D][D / 2])
{
	#pragma unroll
	for(int c = 0; c < D; ++ c) {
		#pragma unroll
		for(int i = 0; i < D / 2; ++ i)
			v[c][i] = p[r0 + i + c * D];
	}
}

// position of the next column's header in the program, given the position right behind this column's touch list
__device__ __forceinline__ int pc_next_column(const int32_t *P, int pc, int nb, int nr)
{
	pc += 2 * nr;
	for(int kb = 1; kb < nb; ++ kb)
		pc += 1 + 2 * P[pc];
	return pc;
}

// s_waitcnt's operand for "at most n vector memory operations outstanding" (gfx9 layout: vmcnt in bits 3:0 and 15:14; expcnt
// and lgkmcnt left at their maxima: not waited for)
constexpr int simt_wait_imm(int n) { return ((n > 63)? 63 : n) % 16 | 7 << 4 | 15 << 8 | ((n > 63)? 63 : n) / 16 << 14; }

// Development aid (SLAMPP_HIP_STAGE_TIMING): clock samples of thread 0 of the workgroup in the middle of the grid.  Returns where
// the launch's record goes, or 0 (another thread, no buffer, or the buffer's 4096 launch records are taken: later launches go
// unrecorded), with the first sample taken; SIMT_TICK() adds one to the caller's p_tm / n_tm, up to 32 a record.
__device__ __forceinline__ long long *simt_timing_begin(long long *p_timing, int &n_tm)
{
	long long *p_tm = 0;
	if(p_timing && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) {
		const unsigned long long n_tm_record = atomicAdd((unsigned long long*)p_timing, 1ull);
		p_tm = (n_tm_record < 4096)? p_timing + 1 + 32 * n_tm_record : 0;
		if(p_tm)
			p_tm[n_tm ++] = wall_clock64();
	}
	return p_tm;
}
#define SIMT_TICK() do { if(p_tm && n_tm < 32) p_tm[n_tm ++] = wall_clock64(); } while(0)

// workgroups of a kernel the device holds at a time: 0 on any error, with the error state cleared
static int simt_resident_workgroups(const void *p_kernel, int n_threads, int n_lds_bytes)
{
	int n_device = 0, n_cus = 0, n_blocks = 0;
	if(!p_kernel || n_lds_bytes < 0 || hipGetDevice(&n_device) != hipSuccess ||
	   hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, n_device) != hipSuccess ||
	   hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_blocks, p_kernel, n_threads, size_t(n_lds_bytes)) != hipSuccess) {
		(void)hipGetLastError();
		return 0;
	}
	return (n_cus > 0 && n_blocks > 0)? n_cus * n_blocks : 0;
}

// A chunk's table (forward or backward) from memory to LDS, one wave: eight loads in flight a lane before the first is waited for.  (A loop of one load
// and one store an entry is compiled to a wait per load: 27 trips to memory one after the other for a table of 1 700 entries, some
// 6 us in front of the first column of every wave.)  n_lane: 0 .. 63
__device__ __forceinline__ void simt_stage_table(long long *p_dst, const long long *__restrict__ p_src, int n_entries, int n_lane)
{
	enum { N_FLIGHT = 8 };
	for(int n_base = 0; n_base < n_entries; n_base += N_FLIGHT * 64) { // (wave-uniform trip count)
		long long v[N_FLIGHT];
		#pragma unroll
		for(int u = 0; u < N_FLIGHT; ++ u) {
			const int i = n_base + u * 64 + n_lane;
			v[u] = p_src[(i < n_entries)? i : n_entries - 1]; // (no lane masked out: the loads of a trip go out together)
		}
		#pragma unroll
		for(int u = 0; u < N_FLIGHT; ++ u) {
			const int i = n_base + u * 64 + n_lane;
			if(i < n_entries)
				p_dst[i] = v[u];
		}
	}
}

// ---- the column arithmetic of the factor kernels (factor_simt_kernel, factor_simt_kernel_ahead, factor_simt_kernel_branches).
// These kernels store the same bits because they run the code below: the one copy of every sum, in its one order.  What a form
// owns is where a column's Lambda comes from and when (touches, register sets, waits) and who stores the diagonal block.
// P: the shape's program (wave-uniform: scalar loads); T: field f of this lane's task at T[W f]; pc: position in the program.

// blocks L(j,c) of block row j: update of the diagonal block (its lower triangle, in a) and of the right-hand side; the offsets
// of entry e + 1 are fetched while entry e is being worked on, and a block is requested whole before its first product
template <int D, int W>
__device__ __forceinline__ void simt_row_entries(double (&a)[D][D], double (&y)[D], int &pc, int nr, int f_op, int f_y, const int32_t *P,
	const long long *T, const double *L, const double *w)
{
	long long off = 0, yoff = 0;
	if(nr > 0) {
		off = T[W * (f_op + P[pc])];
		yoff = T[W * (f_y + P[pc + 1])];
	}
	for(int e = 0; e < nr; ++ e) {
		pc += 2;
		double c[D][D], yc[D];
		load_block<D>(L + off, c);
		load_column<D>(w + yoff, yc);
		if(e + 1 < nr) {
			off = T[W * (f_op + P[pc])];
			yoff = T[W * (f_y + P[pc + 1])];
		}
		#pragma unroll
		for(int t = 0; t < D; ++ t) {
			#pragma unroll
			for(int r = 0; r < D; ++ r) {
				#pragma unroll
				for(int q = 0; q <= r; ++ q)
					a[r][q] -= c[t][r] * c[t][q];
				y[r] -= c[t][r] * yc[t];
			}
		}
	}
}

// Cholesky of the diagonal block, in place in the lower triangle of a, and its inverse (lower triangular) in x; a pivot that is
// not positive is replaced by one and reported in b_bad
template <int D>
__device__ __forceinline__ void simt_cholesky_inverse(double (&a)[D][D], double (&x)[D][D], bool &b_bad)
{
	double rd[D]; // rd[k] = 1 / L(k,k)
	#pragma unroll
	for(int k = 0; k < D; ++ k) {
		double piv = a[k][k];
		const bool b_neg = !(piv > 0); // also catches NaN
		b_bad = b_bad || b_neg;
		piv = b_neg? 1.0 : piv;
		const double s = simt_rsqrt(piv);
		rd[k] = s;
		a[k][k] = piv * s;
		#pragma unroll
		for(int r = k + 1; r < D; ++ r)
			a[r][k] *= s;
		#pragma unroll
		for(int q = k + 1; q < D; ++ q) {
			#pragma unroll
			for(int r = q; r < D; ++ r)
				a[r][q] -= a[r][k] * a[q][k];
		}
	}
	#pragma unroll
	for(int c = 0; c < D; ++ c) {
		#pragma unroll
		for(int r = 0; r < D; ++ r) {
			if(r < c)
				x[r][c] = 0.0;
			else if(r == c)
				x[r][c] = rd[r];
			else {
				double sum = 0;
				#pragma unroll
				for(int t = c; t < r; ++ t)
					sum += a[r][t] * x[t][c];
				x[r][c] = -sum * rd[r];
			}
		}
	}
}

// yn = inv(L_jj) y, that is y_j = inv(L_jj) (b_j - sum L(j,c) y_c), and zeros above the diagonal of a: the factor block is
// stored whole
template <int D>
__device__ __forceinline__ void simt_forward_substitution(double (&yn)[D], double (&a)[D][D], const double (&x)[D][D], const double (&y)[D])
{
	#pragma unroll
	for(int r = 0; r < D; ++ r) {
		double sum = 0;
		#pragma unroll
		for(int t = 0; t <= r; ++ t)
			sum += x[r][t] * y[t];
		yn[r] = sum;
	}
	#pragma unroll
	for(int r = 0; r < D; ++ r) {
		#pragma unroll
		for(int q = r + 1; q < D; ++ q)
			a[r][q] = 0.0;
	}
}

// Lambda's values of a block below the diagonal from memory: acc[i][q] = element (r0 + i, q), zero where the block is fill-in
// (enc < 0); enc: twice the block's offset in A, the low bit set where it is stored transposed.  LPT lanes per task: a lane
// takes DH = D / LPT rows, from r0
template <int D, int LPT>
__device__ __forceinline__ void simt_load_lambda_block(double (&acc)[(LPT == 2)? D / 2 : D][D], long long enc, int r0, const double *__restrict__ A)
{
	enum { DH = (LPT == 2)? D / 2 : D };
	const double *src = A + ((enc < 0)? 0 : (enc >> 1));
	const bool b_trans = (enc & 1) != 0, b_have = enc >= 0;
	if constexpr(LPT == 1) {
		double v[D][D]; // v[c][r] = stored element (r, c)
		#pragma unroll
		for(int c = 0; c < D; ++ c)
			load_column<D>(src + c * D, v[c]);
		#pragma unroll
		for(int r = 0; r < DH; ++ r) {
			#pragma unroll
			for(int q = 0; q < D; ++ q)
				acc[r][q] = b_have? (b_trans? v[r][q] : v[q][r]) : 0.0;
		}
	} else {
		// element (r0 + i, q) of the block: stored at (r0 + i) + q D, or transposed at q + (r0 + i) D
		#pragma unroll
		for(int i = 0; i < DH; ++ i) {
			#pragma unroll
			for(int q = 0; q < D; ++ q) {
				const double f = src[b_trans? q + (r0 + i) * D : (r0 + i) + q * D];
				acc[i][q] = b_have? f : 0.0;
			}
		}
	}
}

// one block below the diagonal, from its Lambda values in acc: L(i,j) = (Lambda(i,j) - sum L(i,c) L(j,c)^T) inv(L_jj)^T, in two
// steps.  First the update pairs: acc -= L(i,c) L(j,c)^T over the block's np pairs.  np: P[pc ++] as read by the caller in front of
// the block's Lambda values (the order the scalar loads have always had)
template <int D, int W, int LPT>
__device__ __forceinline__ void simt_update_pairs(double (&acc)[(LPT == 2)? D / 2 : D][D], int &pc, int np, int f_op, int r0, const int32_t *P,
	const long long *T, const double *L)
{
	enum { DH = (LPT == 2)? D / 2 : D };
	{
		long long off_a = 0, off_b = 0;
		if(np > 0) {
			off_a = T[W * (f_op + P[pc])];
			off_b = T[W * (f_op + P[pc + 1])];
		}
		for(int e = 0; e < np; ++ e) {
			pc += 2;
			double ca[D][DH], cb[D][D]; // ca[t][i] = L(i,c) element (r0 + i, t)
			if constexpr(LPT == 1) {
				double full[D][D];
				load_block<D>(L + off_a, full);
				#pragma unroll
				for(int t = 0; t < D; ++ t) {
					#pragma unroll
					for(int i = 0; i < DH; ++ i)
						ca[t][i] = full[t][i];
				}
			} else
				load_half_rows<D>(L + off_a, r0, ca);
			load_block<D>(L + off_b, cb);
			if(e + 1 < np) {
				off_a = T[W * (f_op + P[pc])];
				off_b = T[W * (f_op + P[pc + 1])];
			}
			#pragma unroll
			for(int t = 0; t < D; ++ t) {
				#pragma unroll
				for(int i = 0; i < DH; ++ i) {
					#pragma unroll
					for(int q = 0; q < D; ++ q)
						acc[i][q] -= ca[t][i] * cb[t][q];
				}
			}
		}
	}
}

// then the product with inv(L_jj)^T (x) and the stores of the lane's DH rows to p_out.  (factor_simt_kernel, simt_kernel.hip, has
// this nest written out for odd D, where no other form exists and D = 7 sits at the end of the register file: a change here is a
// change there)
template <int D, int LPT>
__device__ __forceinline__ void simt_block_product(const double (&acc)[(LPT == 2)? D / 2 : D][D], const double (&x)[D][D], int r0, double *p_out)
{
	enum { DH = (LPT == 2)? D / 2 : D };
	// out = acc inv(L_jj)^T: out[i][q] = sum_{t <= q} acc[i][t] x[q][t] (x[r][c] = element (r, c) of the inverse)
	#pragma unroll
	for(int q = 0; q < D; ++ q) {
		double out[DH];
		#pragma unroll
		for(int i = 0; i < DH; ++ i) {
			double sum = 0;
			#pragma unroll
			for(int t = 0; t <= q; ++ t)
				sum += acc[i][t] * x[q][t];
			out[i] = sum;
		}
		if(DH % 2 == 0 && D % 2 == 0) {
			#pragma unroll
			for(int i = 0; i < DH; i += 2)
				*reinterpret_cast<double2*>(p_out + r0 + i + q * D) = double2{out[i], out[i + 1]};
		} else {
			#pragma unroll
			for(int i = 0; i < DH; ++ i)
				p_out[r0 + i + q * D] = out[i];
		}
	}
}

// ---- the column arithmetic of the backward kernels (backward_simt_kernel, backward_simt_ahead_kernel): x_j = L_jj^-T (y_j -
// sum_i L(i,j)^T x_i).  The same rule: one copy here, the forms own the fetches and the waits.

// 1 / d, refined twice
__device__ __forceinline__ double simt_refined_rcp(double d)
{
	double r = __builtin_amdgcn_rcp(d);
	r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
	r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
	return r;
}

// x of column n_local of the task, from the wave's LDS (s_x: this lane's slot)
template <int D, int W>
__device__ __forceinline__ void simt_local_x(double (&xi)[D], const double *s_x, int n_local)
{
	#pragma unroll
	for(int r = 0; r < D; ++ r)
		xi[r] = s_x[(n_local * D + r) * W];
}

// acc -= L(i,j)^T x_i; c[q][r] = L(i,j)(r, q)
template <int D>
__device__ __forceinline__ void simt_backward_block(double (&acc)[D], const double (&c)[D][D], const double (&xi)[D])
{
	#pragma unroll
	for(int q = 0; q < D; ++ q) {
		#pragma unroll
		for(int r = 0; r < D; ++ r)
			acc[q] -= c[q][r] * xi[r];
	}
}

// x = L_jj^-T acc; a[q][r] = L_jj(r, q) for r > q, rd[q] = 1 / L_jj(q, q).  (bwd_ahead_solve, simt_kernel.hip, has these six lines
// written out, with the reciprocals on the diagonal of its set: a change here is a change there)
template <int D>
__device__ __forceinline__ void simt_solve_transposed(double (&x)[D], const double (&acc)[D], const double (&a)[D][D], const double (&rd)[D])
{
	#pragma unroll
	for(int q = D - 1; q >= 0; -- q) {
		double sum = acc[q];
		#pragma unroll
		for(int r = q + 1; r < D; ++ r)
			sum -= a[q][r] * x[r];
		x[q] = sum * rd[q];
	}
}

// x of column ci of the task to the wave's LDS, for the task's columns still to come
template <int D, int W>
__device__ __forceinline__ void simt_store_local_x(double *s_x, int ci, const double (&x)[D])
{
	#pragma unroll
	for(int q = 0; q < D; ++ q)
		s_x[(ci * D + q) * W] = x[q];
}

// x to the permuted vector (p_w) and to the solution in the caller's order (p_x_out)
template <int D>
__device__ __forceinline__ void simt_store_x(double *p_w, double *p_x_out, const double (&x)[D])
{
	if(D % 2 == 0) {
		#pragma unroll
		for(int q = 0; q < D; q += 2) {
			*reinterpret_cast<double2*>(p_w + q) = double2{x[q], x[q + 1]};
			*reinterpret_cast<double2*>(p_x_out + q) = double2{x[q], x[q + 1]};
		}
	} else {
		#pragma unroll
		for(int q = 0; q < D; ++ q) {
			p_w[q] = x[q];
			p_x_out[q] = x[q];
		}
	}
}
