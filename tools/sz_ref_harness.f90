! SZCC_Cash of the compiled reference (source/szcounts.f90) at listed nuisance
! points: the recorded outputs of tests/golden/sz/sz_fixture.tar.xz (inputs:
! tools/sz_make_fixture.py).
!
! The reference's own SZLikelihood_Add reads the options from an ini and its
! SZ_init the four data files, and its own LogLike is called through the
! likelihood it adds.  Theory%sigma_R is filled from a small analytic sigma(R)
! table (sz_harness_sigma below, restated in tests/sz_fixture.py) through the
! reference's own TCubicSpline.
!
! Build against the reference objects that build() leaves under oracle/_ref/obj
! (FC, OPENBLAS and OPENBLAS_DIR as in oracle/Makefile), from the repository root:
!
!   (cd oracle/_ref/obj && $FC -cpp -O2 -w -c ../../../tools/sz_ref_harness.f90 -o sz_ref_harness.o \
!      && objcopy --redefine-syms=../blas.syms sz_ref_harness.o) && \
!   $FC -o oracle/_ref/sz_ref_harness oracle/_ref/obj/sz_ref_harness.o \
!      $(ls oracle/_ref/obj/*.o | grep -v -e harness -e native -e bench) $OPENBLAS -Wl,-rpath,$OPENBLAS_DIR
!
! and run it inside a dataset's directory, which holds a data/ of its own (the
! reference opens data/SZ_cat.txt, data/SZ_thetas.txt, data/SZ_skyfracs.txt,
! data/SZ_ylims.txt and data/SZ.paramnames by those names):
!
!   (cd DIR/syn_inside && ../../oracle/_ref/sz_ref_harness sz_ref.ini cases.txt ref.txt row.txt info.txt)
!
! cases.txt: H0 omegam omegav omegak w0 ns ombh2 / nR lnR_min lnR_max / ncase /
! one line of the five nuisance values per case.  ref.txt receives -lnL per
! case; row.txt the theory row those inputs imply ([H0, ns, ombh2, E(z_j),
! dA(z_j), grid(m, j) z-major], one number a line) from the reference's public
! Eh, dA and get_grid after its own cosmopar set-up; info.txt the loader
! quantities: nsteps_z, nsteps_m, Nz, Ny + 1, steps_z, then DNcat by rows.
! steps_z and DNcat are private to the reference's routines and modules, so
! they are formed here by this file's own lines in the reference's types
! (default-real literals widened to double) and order; a wrong one shows in
! -lnL, which the reference evaluates with its own.  The compiled reference
! counts a last catalogue row at or above the threshold twice (see below); the
! "total cat" line it prints shows that, and the counts here follow it.
module sz_harness_stub
    use settings
    implicit none
    contains

    real(mcp) function sz_harness_sigma(R)
    real(mcp), intent(in) :: R
    sz_harness_sigma = 0.8_mcp*(R/8._mcp)**(-0.55_mcp)*exp(-(R - 8._mcp)/60._mcp)
    end function sz_harness_sigma

    real(mcp) function sz_harness_next_z(zi, binz)
    real(mcp), intent(in) :: zi, binz
    real(mcp) :: hr, step
    hr = real(0.2, mcp)
    if (zi < hr) then
        step = real(1.e-3, mcp)
    else if (zi <= 1._mcp) then
        step = real(1.e-2, mcp)
    else
        step = binz
    end if
    sz_harness_next_z = zi + step
    end function sz_harness_next_z

end module sz_harness_stub

program sz_ref_harness
    use settings
    use GeneralTypes
    use CosmologyTypes
    use CosmoTheory
    use Likelihood_Cosmology
    use cosmology, only: Eh, dA
    use numbercounts, only: get_grid
    use szcounts
    use sz_harness_stub
    implicit none
    character(len=512) :: ininame, casefile, outfile, rowfile, infofile
    Type(TSettingIni) :: Ini
    Type(TLikelihoodList) :: List
    Type(CMBParams) :: CMB
    Type(TCosmoTheoryPredictions), target :: Theory
    class(TDataLikelihood), pointer :: Like
    logical :: bad
    integer, parameter :: Nq = 5
    integer :: ncase, i, j, k, u, uo, nR, nzs, nm, ncat, ios, ii, Nz
    real(mcp) :: omm, lnRmin, lnRmax, v, nuis(5), zi, binz, minz, maxz, lnm, c1, c2, c3, norm, l1, l3
    real(mcp) :: logq(Nq), zlo, zhi, qlo, qhi, dlogq, dzb, zmaxs
    real(mcp), allocatable :: Zc(:), DNc(:,:)
    real(mcp), allocatable :: Rs(:), sig(:), sz(:), sm(:), grid(:,:), cat(:,:)
    real(mcp), parameter :: dlnm = 0.05_mcp

    call get_command_argument(1, ininame)
    call get_command_argument(2, casefile)
    call get_command_argument(3, outfile)
    call get_command_argument(4, rowfile)
    call get_command_argument(5, infofile)
    Feedback = 0
    DataDir = 'data/'
    call Ini%Open(trim(ininame), bad, .false.)
    if (bad) stop 'cannot open the ini'
    call SZLikelihood_Add(List, Ini)
    if (List%Count /= 1) stop 'SZLikelihood_Add added no likelihood'
    Like => List%Item(1)

    open(newunit=u, file=trim(casefile), status='old')
    CMB%omb = 0
    CMB%omnu = 0
    read(u,*) CMB%H0, omm, CMB%omv, CMB%omk, CMB%w, CMB%InitPower(ns_index), CMB%ombh2
    CMB%omc = omm
    read(u,*) nR, lnRmin, lnRmax
    read(u,*) ncase
    allocate(Rs(nR), sig(nR))
    do i = 1, nR
        Rs(i) = exp(lnRmin + (lnRmax - lnRmin)*(i - 1)/(nR - 1))
        sig(i) = sz_harness_sigma(Rs(i))
    end do
    allocate(Theory%sigma_R)
    call Theory%sigma_R%Init(Rs, sig)
    Theory%sigma_8 = sz_harness_sigma(8._mcp)

    open(newunit=uo, file=trim(outfile), status='replace')
    select type (Like)
    class is (TCosmologyLikelihood)
        do i = 1, ncase
            read(u,*) (nuis(k), k=1,5)
            v = Like%LogLike(CMB, Theory, nuis)
            write(uo,'(ES25.17)') v
        end do
    class default
        stop 'not a cosmology likelihood'
    end select
    close(uo)
    close(u)

    ! the z bins and the steps in z and ln M (SZ_init :1669-1672, deltaN_yz :649-694)
    dzb = 0.1d0
    zmaxs = real(1., mcp)
    Nz = int((zmaxs - 0.d0)/dzb) + 1
    allocate(Zc(Nz), DNc(Nz, Nq))
    do i = 0, Nz - 1
        Zc(i + 1) = 0.d0 + i*dzb + 0.5_mcp*dzb
    end do
    Zc(1) = Zc(1) + real(1.e-8, mcp)
    binz = Zc(2) - Zc(1)
    minz = Zc(1) - 0.5_mcp*binz
    maxz = Zc(Nz) + 0.5_mcp*binz
    if (minz < 0) minz = 0
    zi = minz
    nzs = 0
    do while (zi <= maxz)
        zi = sz_harness_next_z(zi, binz)
        nzs = nzs + 1
    end do
    nm = (real(37., mcp) - real(31., mcp))/dlnm
    allocate(sz(nzs), sm(nm), grid(nm, nzs))
    zi = minz
    do i = 1, nzs
        sz(i) = zi
        zi = sz_harness_next_z(zi, binz)
    end do
    if (sz(1) == 0) sz(1) = real(1.e-5, mcp)
    lnm = real(31., mcp)
    do i = 1, nm
        sm(i) = lnm + dlnm/real(2., mcp)
        lnm = lnm + dlnm
    end do

    ! the row: cosmopar, normgrowth and the sigma(R) pointer are as the last LogLike left them
    grid = 0
    call get_grid(nzs, nm, sz, sm, grid)
    open(newunit=uo, file=trim(rowfile), status='replace')
    write(uo,'(ES25.17)') CMB%H0, CMB%InitPower(ns_index), CMB%ombh2
    do j = 1, nzs
        write(uo,'(ES25.17)') Eh(sz(j))
    end do
    do j = 1, nzs
        write(uo,'(ES25.17)') dA(sz(j))
    end do
    do j = 1, nzs
        write(uo,'(ES25.17)') grid(:, j)
    end do
    close(uo)

    ! the catalogue counts (SZ_init :1573-1608, 1743-1797)
    open(newunit=u, file='data/SZ_cat.txt', status='old')
    ncat = 0
    do
        read(u,*,iostat=ios) c1, c2, c3
        if (ios /= 0) exit
        if (c3 >= real(6., mcp)) ncat = ncat + 1
    end do
    rewind(u)
    allocate(cat(ncat + 1, 2))
    ii = 0
    l1 = 0
    l3 = 0
    do
        read(u,*,iostat=ios) c1, c2, c3
        if (ios /= 0) exit
        l1 = c1
        l3 = c3
        if (c3 >= real(6., mcp)) then
            ii = ii + 1
            cat(ii, 1) = c1
            cat(ii, 2) = c3
        end if
    end do
    close(u)
    ! the reference's second pass (:1600-1608) reads one line more than the file
    ! holds; that read fails and leaves the last row's values in place, so a
    ! last row at or above the threshold enters the catalogue twice
    if (l3 >= real(6., mcp)) then
        ncat = ncat + 1
        cat(ncat, 1) = l1
        cat(ncat, 2) = l3
    end if
    dlogq = real(0.25, mcp)
    zi = real(0.7, mcp) + dlogq/real(2., mcp)
    do j = 1, Nq
        logq(j) = zi
        zi = zi + dlogq
    end do
    DNc = 0
    zlo = 0.d0
    zhi = zlo + dzb
    do i = 1, Nz
        do j = 1, Nq
            qlo = 10.d0**(logq(j) - dlogq/real(2., mcp))
            qhi = 10.d0**(logq(j) + dlogq/real(2., mcp))
            if (j == Nq) qlo = 10.d0**(logq(Nq - 1) + dlogq/real(2., mcp))
            do ii = 1, ncat
                if (cat(ii, 1) >= zlo .and. cat(ii, 1) < zhi .and. cat(ii, 2) >= qlo .and. &
                    (j == Nq .or. cat(ii, 2) < qhi)) DNc(i, j) = DNc(i, j) + real(1., mcp)
            end do
        end do
        zlo = zlo + dzb
        zhi = zhi + dzb
    end do
    ! clusters without a redshift: the missing-redshift limits come from 10.**x with x double
    do j = 1, Nq
        qlo = real(10., mcp)**(logq(j) - dlogq/real(2., mcp))
        qhi = real(10., mcp)**(logq(j) + dlogq/real(2., mcp))
        if (j == Nq) qlo = real(10., mcp)**(logq(Nq - 1) + dlogq/real(2., mcp))
        do ii = 1, ncat
            if (cat(ii, 1) == -1 .and. cat(ii, 2) >= qlo .and. (j == Nq .or. cat(ii, 2) < qhi)) then
                norm = 0
                do k = 1, Nz
                    norm = norm + DNc(k, j)
                end do
                DNc(:, j) = DNc(:, j)*(norm + 1.d0)/norm
            end if
        end do
    end do
    open(newunit=uo, file=trim(infofile), status='replace')
    write(uo,'(4I8)') nzs, nm, Nz, Nq
    write(uo,'(ES25.17)') sz
    do i = 1, Nz
        write(uo,'(5ES25.17)') DNc(i, :)
    end do
    close(uo)
end program
