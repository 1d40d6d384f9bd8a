! WL_LnLike of the compiled reference (source/wl.f90) at listed nuisance points:
! the recorded outputs of tests/golden/wl/wl_fixture.tar.xz (inputs:
! tools/wl_make_fixture.py).
!
! The reference's own WLLikelihood_Add reads the options and the dataset from
! an ini, and its own LogLike is called through the likelihood it adds.  The
! calculator it asks for distances and H(z) is a stub that returns the case
! file's tabulated values; Theory%MPK, NL_MPK and their Weyl pair are filled
! from a small analytic (log kh, z) grid (wl_harness_pk below, restated in
! tests/wl_fixture.py) through the reference's own InitExtrap.
!
! Build against the reference objects that build() leaves under oracle/_ref/obj
! (FC, OPENBLAS and OPENBLAS_DIR as in oracle/Makefile), from the repository root:
!
!   (cd oracle/_ref/obj && $FC -cpp -O2 -w -c ../../../tools/wl_ref_harness.f90 -o wl_ref_harness.o \
!      && objcopy --redefine-syms=../blas.syms wl_ref_harness.o) && \
!   $FC -o oracle/_ref/wl_ref_harness oracle/_ref/obj/wl_ref_harness.o \
!      $(ls oracle/_ref/obj/*.o | grep -v -e harness -e native -e bench) $OPENBLAS -Wl,-rpath,$OPENBLAS_DIR
!
! and run it inside a dataset's directory (the file names in wl.ini and in the
! dataset are relative to it); add a repeat count to time the evaluations:
!
!   (cd DIR/syn_all && ../../oracle/_ref/wl_ref_harness wl.ini cases.txt ref.txt row.txt info.txt [repeats])
!
! cases.txt: H0 omdm omb / nk nzg logkh_min logkh_max zg_max / nz / chis(1:nz) /
! Hs(1:nz) / nl / l(1:nl) / ncase nn / one line of nn nuisance values per case.
! ref.txt receives -lnL per case; row.txt the theory row those inputs imply
! ([h, omm, chis, Hs, D_growth, P(nl, nz)], one number a line), formed by this
! file's own lines from kh = (l + 1/2) / chi / h and PowerAtArr at the l of the
! case file; info.txt the loader quantities the reference exposes:
! first_theta_bin_used (the least theta bin of used_items) and used_items.
! ls_cl and ls_bessel are private components of WLLikelihood and are not
! printed: the l of the case file are the project's own ls_cl, and a wrong
! ls_cl or ls_bessel shows in -lnL (the reference evaluates with its own).
module wl_harness_stub
    use settings
    use Calculator_Cosmology
    implicit none

    type, extends(TCosmologyCalculator) :: TStubCalculator
        real(mcp), allocatable :: z(:), chis(:), Hs(:)
    contains
    procedure :: ComovingRadialDistanceArr => Stub_ComovingRadialDistanceArr
    procedure :: Hofz => Stub_Hofz
    end type TStubCalculator

    contains

    subroutine Stub_ComovingRadialDistanceArr(this, z, arr, n)
    class(TStubCalculator) :: this
    integer, intent(in) :: n
    real(mcp), intent(IN) :: z(n)
    real(mcp), intent(out) :: arr(n)
    if (n /= size(this%chis)) stop 'stub: wrong number of redshifts'
    arr = this%chis
    end subroutine Stub_ComovingRadialDistanceArr

    real(mcp) function Stub_Hofz(this, z)
    class(TStubCalculator) :: this
    real(mcp), intent(IN) :: z
    integer :: i(1)
    i = minloc(abs(this%z - z))
    if (this%z(i(1)) /= z) stop 'stub: Hofz off the table'
    Stub_Hofz = this%Hs(i(1))
    end function Stub_Hofz

    ! ln P(ln kh, z): which = 1 MPK, 2 NL_MPK, 3 MPK_WEYL, 4 NL_MPK_WEYL
    real(mcp) function wl_harness_pk(which, lk, z)
    integer, intent(in) :: which
    real(mcp), intent(in) :: lk, z
    real(mcp) :: k, v
    k = exp(lk)
    v = 10._mcp + lk - 1.5_mcp*log(1 + (k/0.02_mcp)**2) - 2*log(1 + 0.6_mcp*z)
    if (which == 2 .or. which == 4) v = v + 0.5_mcp*log(1 + (k/0.3_mcp)**2)/(1 + z)
    if (which >= 3) v = v - 16._mcp + 0.3_mcp*z
    wl_harness_pk = v
    end function wl_harness_pk

end module wl_harness_stub

program wl_ref_harness
    use settings
    use GeneralTypes
    use CosmologyTypes
    use CosmoTheory
    use Likelihood_Cosmology
    use wl
    use wl_harness_stub
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
    integer :: ncase, nn, i, j, k, u, uo, nz, nk, nzg, nrep, rep, which, ix, nl, first
    integer(8) :: c0, c1, rate
    real(mcp) :: lkmin, lkmax, zgmax, v, h, omm, kh, khmin, khmax, p0
    real(mcp), allocatable :: lk(:), zg(:), tab(:,:), nuis(:), Dg(:), kharr(:), zarr(:), powers(:), prow(:)
    integer, allocatable :: ls(:)

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
    call Ini%Open(trim(ininame), bad, .false.)
    if (bad) stop 'cannot open the ini'
    call WLLikelihood_Add(List, Ini)
    if (List%Count /= 1) stop 'WLLikelihood_Add added no likelihood'
    Like => List%Item(1)

    open(newunit=u, file=trim(casefile), status='old')
    read(u,*) CMB%H0, CMB%omdm, CMB%omb
    read(u,*) nk, nzg, lkmin, lkmax, zgmax
    read(u,*) nz
    allocate(Stub%z(nz), Stub%chis(nz), Stub%Hs(nz), Dg(nz), kharr(nz), zarr(nz), powers(nz), prow(nz))
    read(u,*) (Stub%chis(k), k=1,nz)
    read(u,*) (Stub%Hs(k), k=1,nz)
    read(u,*) nl
    allocate(ls(nl))
    read(u,*) (ls(k), k=1,nl)
    read(u,*) ncase, nn
    allocate(nuis(nn))

    allocate(lk(nk), zg(nzg), tab(nk, nzg))
    do i = 1, nk
        lk(i) = lkmin + (lkmax - lkmin)*(i - 1)/(nk - 1)
    end do
    do j = 1, nzg
        zg(j) = zgmax*(j - 1)/(nzg - 1)
    end do
    allocate(Theory%MPK, Theory%NL_MPK, Theory%MPK_WEYL, Theory%NL_MPK_WEYL)
    do which = 1, 4
        do j = 1, nzg
            do i = 1, nk
                tab(i, j) = wl_harness_pk(which, lk(i), zg(j))
            end do
        end do
        if (which == 1) call Theory%MPK%InitExtrap(lk, zg, tab)
        if (which == 2) call Theory%NL_MPK%InitExtrap(lk, zg, tab)
        if (which == 3) call Theory%MPK_WEYL%InitExtrap(lk, zg, tab)
        if (which == 4) call Theory%NL_MPK_WEYL%InitExtrap(lk, zg, tab)
    end do

    open(newunit=uo, file=trim(outfile), status='replace')
    select type (Like)
    class is (WLLikelihood)
        if (Like%num_z_p /= nz) stop 'case file and dataset disagree on num_z_p'
        Stub%z = Like%z_p
        Like%Calculator => Stub
        do i = 1, ncase
            read(u,*) (nuis(k), k=1,nn)
            call system_clock(c0, rate)
            do rep = 1, nrep
                v = Like%LogLike(CMB, Theory, nuis)
            end do
            call system_clock(c1)
            write(uo,'(ES25.17)') v
            if (nrep > 1) write(*,'("case ",I2,": ",F10.3," ms per evaluation")') i, &
                1d3 * real(c1 - c0, 8) / real(rate, 8) / nrep
        end do
        close(uo)

        first = Like%num_theta_bins
        if (Like%num_used > 0) first = minval(Like%used_items(:, 4))
        open(newunit=uo, file=trim(infofile), status='replace')
        write(uo,'(2I8)') first, Like%num_used
        do i = 1, Like%num_used
            write(uo,'(4I6)') Like%used_items(i, :)
        end do
        close(uo)

        ! the theory row: PK chosen as calc_theory chooses it (:452-464)
        if (Like%use_non_linear) then
            if (Like%use_weyl) then
                PK => Theory%NL_MPK_WEYL
            else
                PK => Theory%NL_MPK
            end if
        else
            if (Like%use_weyl) then
                PK => Theory%MPK_WEYL
            else
                PK => Theory%MPK
            end if
        end if
        h = CMB%H0/100
        omm = CMB%omdm + CMB%omb
        p0 = Theory%MPK%PowerAt(0.01d0, 0.d0)
        do j = 1, nz
            Dg(j) = sqrt(Theory%MPK%PowerAt(0.01d0, Like%z_p(j))/p0)
        end do
        khmin = exp(PK%x(1))
        khmax = exp(PK%x(PK%nx))
        open(newunit=uo, file=trim(rowfile), status='replace')
        write(uo,'(ES25.17)') h, omm
        write(uo,'(ES25.17)') Stub%chis
        write(uo,'(ES25.17)') Stub%Hs
        write(uo,'(ES25.17)') Dg
        write(uo,'(2ES25.17)') khmin, khmax
        do i = 1, nl
            ix = 0
            do j = 1, nz
                kh = (ls(i) + 0.5) / Stub%chis(j) / h
                if (kh >= khmin .and. kh <= khmax) then
                    ix = ix + 1
                    zarr(ix) = Like%z_p(j)
                    kharr(ix) = kh
                end if
            end do
            call PK%PowerAtArr(kharr, zarr, ix, powers)
            ix = 0
            do j = 1, nz
                kh = (ls(i) + 0.5) / Stub%chis(j) / h
                if (kh >= khmin .and. kh <= khmax) then
                    ix = ix + 1
                    prow(j) = powers(ix)
                else
                    prow(j) = 0
                end if
            end do
            write(uo,'(ES25.17)') prow
        end do
        close(uo)
    class default
        stop 'not a WLLikelihood'
    end select
end program
