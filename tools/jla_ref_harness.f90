! JLA_alpha_beta_like of the compiled reference at listed points: the recorded
! outputs of tests/golden/jla (inputs: tools/jla_make_fixture.py).
!
! Build against the reference objects that build() leaves under oracle/_ref/obj
! (FC, OPENBLAS and OPENBLAS_DIR as in oracle/Makefile), from the repository root:
!
!   (cd oracle/_ref/obj && $FC -cpp -O2 -w -c ../../../tools/jla_ref_harness.f90 -o jla_ref_harness.o \
!      && objcopy --redefine-syms=../blas.syms jla_ref_harness.o) && \
!   $FC -o oracle/_ref/jla_ref_harness oracle/_ref/obj/jla_ref_harness.o \
!      $(ls oracle/_ref/obj/*.o | grep -v -e harness -e native -e bench) $OPENBLAS -Wl,-rpath,$OPENBLAS_DIR
!
! and run it inside a dataset's directory (the file names in jla.dataset are
! relative to it); add a repeat count to time the evaluations:
!
!   (cd DIR/syn37 && ../../oracle/_ref/jla_ref_harness jla.dataset cases.txt ref.txt [repeats])
!
! The results go to a file: the reference prints its own error lines on stdout.
program jla_ref_harness
    use settings
    use JLA
    implicit none
    character(len=512) :: dsname, casefile, outfile, arg
    integer :: ncase, i, k, u, uo, rep, nrep
    integer(8) :: c0, c1, rate
    real(mcp) :: alpha, beta, v
    real(mcp), allocatable :: mu(:)
    call get_command_argument(1, dsname)
    call get_command_argument(2, casefile)
    call get_command_argument(3, outfile)
    nrep = 1
    if (command_argument_count() > 3) then
        call get_command_argument(4, arg)
        read(arg, *) nrep
    end if
    Feedback = 0
    call read_jla_dataset(trim(dsname))
    call jla_prep
    allocate(mu(nsn))
    open(newunit=u, file=trim(casefile), status='old')
    open(newunit=uo, file=trim(outfile), status='replace')
    read(u,*) ncase
    do i = 1, ncase
        read(u,*) alpha, beta
        read(u,*) (mu(k), k=1,nsn)
        call system_clock(c0, rate)
        do rep = 1, nrep
            v = JLA_alpha_beta_like(alpha, beta, mu)
        end do
        call system_clock(c1)
        write(uo,'(ES25.17)') v
        if (nrep > 1) write(*,'("case ",I2,": ",F10.3," ms per evaluation")') i, &
            1d3 * real(c1 - c0, 8) / real(rate, 8) / nrep
    end do
    close(uo)
end program
