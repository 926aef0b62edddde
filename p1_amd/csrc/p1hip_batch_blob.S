/* Embeds the gfx950 code object built from p1hip_batch_kernels.hip (Makefile:
   build/p1hip_batch.hsaco) into libp1hip.so, after the scan object of
   p1hip_kernels_blob.S; p1hip.hip loads it with hipModuleLoadData next to
   that one on every device it initialises. */
    .section .rodata
    .balign 4096
    .globl p1hip_batch_co
    .type p1hip_batch_co, @object
p1hip_batch_co:
    .incbin P1HIP_BATCH_CO
    .globl p1hip_batch_co_end
p1hip_batch_co_end:
    .section .note.GNU-stack,"",@progbits
