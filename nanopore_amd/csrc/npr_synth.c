/* npr_synth.c -- the inner loop of nanopore_amd/synth.py::error_channel (synthetic workloads for tests and bench.py; never
 * part of libnprealign.so).  Host C, no GPU.
 *
 * The draws come from the caller's numpy Generator through its bit generator's next_double, in exactly the order the
 * vectorised walk makes them: at every step one transition draw per active read in read order, then one match-emission
 * draw per read that took a match, then one insert-emission draw per read that took an insert.  The workloads therefore
 * stay what the seeds made them, and the generator is left in the state the vectorised walk leaves it in.
 *
 * Column t of every read is taken at step t, so the walk writes one row of n bytes per step (op codes and emitted bases,
 * read-major within the row) and npr_synth_gather turns the rows into the per-read concatenations, 64 reads at a time.
 */
#include <stdint.h>

#define OP_M 0
#define OP_I 1
#define OP_D 2

typedef double (*npr_next_double)(void *);

/* Tc[5][4], Mc[4][3], Ic[3]: cumulative thresholds (category = number of thresholds <= u).  op_rows / base_rows: [max_steps][n].
 * lane, state, xpos: scratch of n.  Returns the number of steps, or -1 when reads are still active after max_steps. */
int64_t npr_synth_channel(void *bitgen, npr_next_double next_double, const uint8_t *ref, const int64_t *ref_off, int64_t n,
                          const double *Tc, const double *Mc, const double *Ic, int64_t cap, int64_t max_steps,
                          uint8_t *op_rows, uint8_t *base_rows, int64_t *rlen, int64_t *nops,
                          int64_t *lane, int64_t *state, int64_t *xpos)
{
    int64_t na = 0;
    for (int64_t i = 0; i < n; i++) {
        rlen[i] = 0;
        nops[i] = 0;
        if (ref_off[i + 1] > ref_off[i]) {
            lane[na] = i;
            state[na] = 0;
            xpos[na] = ref_off[i];
            na++;
        }
    }
    int64_t t = 0;
    for (; na > 0; t++) {
        if (t == max_steps)
            return -1;
        uint8_t *ops = op_rows + t * n, *bases = base_rows + t * n;
        for (int64_t i = 0; i < n; i++) {  /* (the rows of finished reads: what the vectorised walk's rows hold there) */
            ops[i] = OP_D;
            bases[i] = 0;
        }
        for (int64_t k = 0; k < na; k++) {
            double u = next_double(bitgen);
            const double *c = Tc + 4 * state[k];
            int s = (u >= c[0]) + (u >= c[1]) + (u >= c[2]) + (u >= c[3]);
            state[k] = s;
            int is_m = s == 0, is_x = s == 1 || s == 3;  /* else an insert (2, 4) */
            /* reads that would overflow their buffers are forced to consume reference */
            if (rlen[lane[k]] >= cap - 1 || t >= 2 * cap - 1) {
                is_x |= !is_m;
            }
            ops[lane[k]] = is_m ? OP_M : is_x ? OP_D : OP_I;
        }
        for (int64_t k = 0; k < na; k++) {
            int64_t i = lane[k];
            if (ops[i] == OP_M) {
                double u = next_double(bitgen);
                const double *c = Mc + 3 * ref[xpos[k]];
                bases[i] = (u >= c[0]) + (u >= c[1]) + (u >= c[2]);
            }
        }
        for (int64_t k = 0; k < na; k++) {
            int64_t i = lane[k];
            if (ops[i] == OP_I) {
                double u = next_double(bitgen);
                bases[i] = (u >= Ic[0]) + (u >= Ic[1]) + (u >= Ic[2]);
            }
        }
        int64_t w = 0;
        for (int64_t k = 0; k < na; k++) {
            int64_t i = lane[k];
            rlen[i] += ops[i] != OP_D;
            xpos[k] += ops[i] != OP_I;
            if (xpos[k] < ref_off[i + 1]) {
                lane[w] = i;
                state[w] = state[k];
                xpos[w] = xpos[k];
                w++;
            } else {
                nops[i] = t + 1;
            }
        }
        na = w;
    }
    return t;
}

/* The rows of npr_synth_channel's `steps` steps -> ops[ops_off[i] ..] (every column of read i) and reads[read_off[i] ..] (the
 * bases of its M and I columns). */
void npr_synth_gather(const uint8_t *op_rows, const uint8_t *base_rows, int64_t n, int64_t steps, const int64_t *nops,
                      const int64_t *ops_off, const int64_t *read_off, uint8_t *ops, uint8_t *reads)
{
    for (int64_t i0 = 0; i0 < n; i0 += 64) {
        int64_t i1 = i0 + 64 < n ? i0 + 64 : n, r[64];
        for (int64_t i = i0; i < i1; i++)
            r[i - i0] = read_off[i];
        for (int64_t t = 0; t < steps; t++) {
            const uint8_t *o = op_rows + t * n, *b = base_rows + t * n;
            for (int64_t i = i0; i < i1; i++) {
                if (t >= nops[i])
                    continue;
                ops[ops_off[i] + t] = o[i];
                if (o[i] != OP_D)
                    reads[r[i - i0]++] = b[i];
            }
        }
    }
}
