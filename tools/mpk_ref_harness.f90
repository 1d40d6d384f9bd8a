! MPK_LnLike and WiggleZ_LnLike of the compiled reference (source/mpk.f90,
! source/wigglez.f90) at listed cosmologies: the recorded outputs of
! tests/golden/mpk/mpk_fixture.tar.xz (inputs: tools/mpk_make_fixture.py).
!
! The reference's own MPKLikelihood_Add and WiggleZLikelihood_Add read the run
! ini and the .dataset files, and its own LogLike is called through the one
! likelihood they add.  The calculator it asks for BAO_D_v is a stub that
! returns the case's D_V whatever the redshift; CMB%H0 is the case's.
! Theory%MPK and Theory%NL_MPK are filled from a small analytic (ln kh, z) grid
! (mpk_harness_pk below, restated in tests/mpk_fixture.py) through the
! reference's own InitExtrap, once per case (the grid's lower edge is a case
! quantity), and exact_z_index points at the dataset's redshift in it.
!
! Build against the reference objects that build() leaves under oracle/_ref/obj
! (FC, OPENBLAS and OPENBLAS_DIR as in oracle/Makefile; -O2 without fast-math,
! as the oracle's), from the repository root:
!
!   (cd oracle/_ref/obj && $FC -cpp -O2 -w -c ../../../tools/mpk_ref_harness.f90 -o mpk_ref_harness.o \
!      && objcopy --redefine-syms=../blas.syms mpk_ref_harness.o) && \
!   $FC -o oracle/_ref/mpk_ref_harness oracle/_ref/obj/mpk_ref_harness.o \
!      $(ls oracle/_ref/obj/*.o | grep -v -e harness -e native -e bench) $OPENBLAS -Wl,-rpath,$OPENBLAS_DIR
!
! and run it inside a dataset's directory (the file names in the ini and in the
! .dataset files are relative to it, and the GiggleZ fiducial files are opened
! as data/gigglezfiducialmodel_matterpower_{a..d}.dat); add a repeat count to
! time the evaluations:
!
!   (cd DIR/NAME && ../../oracle/_ref/mpk_ref_harness ref.ini cases.txt ref.txt row.txt info.txt [repeats])
!
! cases.txt: nk nzg lkmax use_scaling(0/1) / nkb / k(1:nkb), one a line / ncase /
! per case "H0 DV amp tilt lkmin".  The k are the project's own selection of the
! kbands file: MPKLikelihood exposes its own and the harness stops if they
! differ; WiggleZLikelihood is private to its module, and a wrong k there shows
! in -lnL (the reference evaluates with its own).
! The grid of a case is ln kh = lkmin + (lkmax - lkmin)(i - 1)/(nk - 1) and
! z = z_dataset (j - 1)/2, j = 1..nzg (so j = 3 is the dataset's redshift).
! ref.txt receives -lnL per case; row.txt per case a_scl, kh_min = exp(PK%x(1))
! and PowerAt(max(kh_min, a_scl k_i), z) for the kbands used, one number a
! line, formed by this file's own lines; info.txt the loader quantities the
! types expose.  MPK: "np nk 1 0 has_cov 0", the k used, the data vector, the
! sdev column, and the inverse covariance row by row when there is one.
! WiggleZ: "0 nk 0 0 0 1", then DV_fid, the redshift and kmax.
module mpk_harness_stub
    use settings
    use Calculator_Cosmology
    implicit none

    type, extends(TCosmologyCalculator) :: TStubCalculator
        real(mcp) :: DV = 0
    contains
    procedure :: BAO_D_v => Stub_BAO_D_v
    end type TStubCalculator

    contains

    real(mcp) function Stub_BAO_D_v(this, z)
    class(TStubCalculator) :: this
    real(mcp), intent(IN) :: z
    Stub_BAO_D_v = this%DV
    end function Stub_BAO_D_v

    ! ln P(ln kh, z): which = 1 MPK, 2 NL_MPK
    real(mcp) function mpk_harness_pk(which, lk, z, amp, tilt)
    integer, intent(in) :: which
    real(mcp), intent(in) :: lk, z, amp, tilt
    real(mcp) :: k, v
    k = exp(lk)
    v = amp + tilt*lk - 1.5_mcp*log(1 + (k/0.02_mcp)**2) - 2*log(1 + 0.6_mcp*z)
    if (which == 2) v = v + 0.5_mcp*log(1 + (k/0.3_mcp)**2)/(1 + z)
    mpk_harness_pk = v
    end function mpk_harness_pk

end module mpk_harness_stub

program mpk_ref_harness
    use settings
    use GeneralTypes
    use CosmologyTypes
    use CosmoTheory
    use Likelihood_Cosmology
    use MPK_Common
    use mpk
    use wigglez
    use mpk_harness_stub
    implicit none
    character(len=512) :: ininame, casefile, outfile, rowfile, infofile, arg
    Type(TSettingIni) :: Ini
    Type(TLikelihoodList) :: List
    Type(TStubCalculator), target :: Stub
    Type(CMBParams) :: CMB
    Type(TCosmoTheoryPredictions), target :: Theory
    type(TCosmoTheoryPK), pointer :: PK
    class(TDataLikelihood), pointer :: Like
    logical :: bad
    integer :: ncase, i, j, ic, u, uo, ur, ui, nk, nzg, nrep, rep, which, iscl, np, nkb, nr, r
    integer(8) :: c0, c1, rate
    real(mcp) :: lkmin, lkmax, v, amp, tilt, zd, a_scl, khmin, ks
    real(mcp), allocatable :: lk(:), zg(:), tab(:,:), nuis(:), kb(:)

    call get_command_argument(1, ininame)
    call get_command_argument(2, casefile)
    call get_command_argument(3, outfile)
    call get_command_argument(4, rowfile)
    call get_command_argument(5, infofile)
    nrep = 1
    if (command_argument_count() > 5) then
        call get_command_argument(6, arg)
        read(arg, *) nrep
    end if
    Feedback = 0
    DataDir = 'data/'   ! as the driver sets it: %DATASETDIR% and the GiggleZ fiducial files
    call Ini%Open(trim(ininame), bad, .false.)
    if (bad) stop 'cannot open the ini'
    call MPKLikelihood_Add(List, Ini)
    call WiggleZLikelihood_Add(List, Ini)
    if (List%Count /= 1) stop 'the ini must add exactly one likelihood'
    Like => List%Item(1)
    allocate(nuis(0))

    open(newunit=u, file=trim(casefile), status='old')
    read(u,*) nk, nzg, lkmax, iscl
    read(u,*) nkb
    allocate(kb(nkb))
    do i = 1, nkb
        read(u,*) kb(i)
    end do
    read(u,*) ncase
    allocate(lk(nk), zg(nzg), tab(nk, nzg))
    allocate(Theory%MPK, Theory%NL_MPK)

    ! the loader quantities
    open(newunit=ui, file=trim(infofile), status='replace')
    select type (Like)
    class is (MPKLikelihood)
        np = Like%num_mpk_points_use
        if (nkb /= Like%num_mpk_kbands_use) stop 'case file and dataset disagree on the kbands used'
        if (any(kb /= Like%PKData%mpk_k)) stop 'case file and dataset disagree on k'
        write(ui,'(6I6)') np, nkb, 1, 0, merge(1, 0, allocated(Like%PKData%mpk_invcov)), 0
        write(ui,'(ES25.17)') kb
        write(ui,'(ES25.17)') Like%PKData%mpk_P
        write(ui,'(ES25.17)') Like%PKData%mpk_sdev
        if (allocated(Like%PKData%mpk_invcov)) then
            do i = 1, np
                write(ui,'(ES25.17)') Like%PKData%mpk_invcov(i, :)
            end do
        end if
    class is (TCosmologyPKLikelihood)
        ! WiggleZLikelihood is private to its module: only what its parent exposes
        write(ui,'(6I6)') 0, nkb, 0, 0, 0, 1
        write(ui,'(ES25.17)') Like%DV_fid, Like%exact_z(1), Like%kmax
    class default
        stop 'not a TCosmologyPKLikelihood'
    end select
    close(ui)

    open(newunit=uo, file=trim(outfile), status='replace')
    open(newunit=ur, file=trim(rowfile), status='replace')
    select type (Like)
    class is (TCosmologyPKLikelihood)
        Like%Calculator => Stub
        if (.not. allocated(Like%exact_z_index)) allocate(Like%exact_z_index(1))
        Like%exact_z_index(1) = 3
        zd = Like%exact_z(1)
        do j = 1, nzg
            zg(j) = zd*(j - 1)/2
        end do
        do ic = 1, ncase
            read(u,*) CMB%H0, Stub%DV, amp, tilt, lkmin
            do i = 1, nk
                lk(i) = lkmin + (lkmax - lkmin)*(i - 1)/(nk - 1)
            end do
            do which = 1, 2
                do j = 1, nzg
                    do i = 1, nk
                        tab(i, j) = mpk_harness_pk(which, lk(i), zg(j), amp, tilt)
                    end do
                end do
                if (which == 1) call Theory%MPK%InitExtrap(lk, zg, tab)
                if (which == 2) call Theory%NL_MPK%InitExtrap(lk, zg, tab)
            end do
            call system_clock(c0, rate)
            do rep = 1, nrep
                v = Like%LogLike(CMB, Theory, nuis)
            end do
            call system_clock(c1)
            write(uo,'(ES25.17)') v
            if (nrep > 1) write(*,'("case ",I2,": ",F10.4," ms per evaluation")') ic, &
                1d3 * real(c1 - c0, 8) / real(rate, 8) / nrep

            ! the theory row (mpk.f90:296-313, wigglez.f90:534-545)
            if (Like%needs_nonlinear_pk) then
                PK => Theory%NL_MPK
            else
                PK => Theory%MPK
            end if
            if (iscl /= 0) then
                a_scl = Like%compute_scaling_factor(zd, CMB)
            else
                a_scl = 1
            end if
            khmin = exp(PK%x(1))
            write(ur,'(ES25.17)') a_scl, khmin
            do i = 1, nkb
                ks = max(khmin, a_scl*kb(i))
                write(ur,'(ES25.17)') PK%PowerAt(ks, zd)
            end do
        end do
    class default
        stop 'not a TCosmologyPKLikelihood'
    end select
    close(uo)
    close(ur)
    close(u)
end program
