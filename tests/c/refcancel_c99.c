/* refcancel_c99.c -- the canceller's part of include/crsdr.h from strict C99 (gcc -std=c99 -pedantic), linked against libcrsdr.so:
 * the four calls exist with the declared signatures and refuse bad arguments without looking for a device. */
#include <crsdr.h>
#include <stdio.h>

int main(void)
{
    int8_t rows[2 * 64] = {0}, out[2 * 64];
    float coef[2 * 9 * 2], residual[2], phasor[4] = {0, 0, 1, 0};
    int32_t status[2], lag[2] = {0, 0};
    void *p = 0;
    int taps = -1;
    printf("set %d\n", crsdr_plan_set_refcancel(0, 9));
    printf("fetch %d\n", crsdr_plan_fetch_refcancel(0, -1, coef, residual, status));
    printf("buffers %d\n", crsdr_plan_refcancel_buffers(0, &p, &p, &p, &taps));
    printf("taps %d\n", crsdr_refcancel(out, coef, residual, status, rows, 2, 64, lag, phasor, 4, 0u, CRSDR_MEM_HOST));
    lag[1] = 33;
    printf("lag %d\n", crsdr_refcancel(out, coef, residual, status, rows, 2, 64, lag, phasor, 9, 0u, CRSDR_MEM_HOST));
    printf("error: %s\n", crsdr_last_error());
    return 0;
}
