// simt_device.inl -- what the lane-per-task kernels share (simt_kernel.hip, simt_factor_ahead.hip): a lane's loads and stores of
// its own D x D blocks, the reciprocal square root, the walk through a shape's program.  Included inside namespace slampp.

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
