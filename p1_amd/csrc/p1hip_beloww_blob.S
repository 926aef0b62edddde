/* Embeds the gfx950 code object built from p1hip_beloww_kernels.hip (Makefile:
   build/p1hip_beloww.hsaco) into libp1hip.so, after the scan, batch, below and
   below batch objects of p1hip_kernels_blob.S, p1hip_batch_blob.S,
   p1hip_below_blob.S and p1hip_belowb_blob.S; p1hip.hip loads it with
   hipModuleLoadData next to those on every device it initialises. */
    .section .rodata
    .balign 4096
    .globl p1hip_beloww_co
    .type p1hip_beloww_co, @object
p1hip_beloww_co:
    .incbin P1HIP_BELOWW_CO
    .globl p1hip_beloww_co_end
p1hip_beloww_co_end:
    .section .note.GNU-stack,"",@progbits
