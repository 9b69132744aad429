// Context switch for the SIMT emulator's fibers (tests only). x86-64 SysV.
__asm__(
    ".text\n"
    ".globl hipemu_switch\n"
    ".type hipemu_switch,@function\n"
    "hipemu_switch:\n"
    "    pushq %rbp\n"
    "    pushq %rbx\n"
    "    pushq %r12\n"
    "    pushq %r13\n"
    "    pushq %r14\n"
    "    pushq %r15\n"
    "    movq %rsp, (%rdi)\n"
    "    movq %rsi, %rsp\n"
    "    popq %r15\n"
    "    popq %r14\n"
    "    popq %r13\n"
    "    popq %r12\n"
    "    popq %rbx\n"
    "    popq %rbp\n"
    "    ret\n"
    ".size hipemu_switch,.-hipemu_switch\n");

// Largest dynamic-LDS grant the hipFuncSetAttribute stub allows (tests of the launchers' refusal paths); negative = no limit.
// Setting it restarts the two records a test reads to see WHICH kernel a launcher took: grants refused, largest LDS launched.
extern "C" {
int hipemu_lds_limit = -1, hipemu_lds_refusals = 0, hipemu_max_launch_lds = 0;
void hipemu_set_lds_limit(int bytes) { hipemu_lds_limit = bytes; hipemu_lds_refusals = 0; hipemu_max_launch_lds = 0; }
}
