! jla_LnLike of the compiled reference with JLA_marginalize = T at listed
! distance moduli: the recorded outputs of tests/golden/jla/jla_marge.tar.xz
! (inputs: tools/jla_make_fixture.py --archive marge).
!
! The reference's own JLALikelihood_Add reads the options and the dataset from
! an ini, and its own jla_LnLike is called through the likelihood it adds; the
! calculator it asks for distances is a stub that returns, call by call,
! D_A = 10^(mu_i / 5) / ((1 + zhel_i)(1 + zcmb_i)) of the case's moduli, so
! that jla_LnLike's lumdists are those moduli.
!
! Build against the reference objects that build() leaves under oracle/_ref/obj
! (FC, OPENBLAS and OPENBLAS_DIR as in oracle/Makefile), from the repository root:
!
!   (cd oracle/_ref/obj && $FC -cpp -O2 -w -c ../../../tools/jla_marge_ref_harness.f90 -o jla_marge_ref_harness.o \
!      && objcopy --redefine-syms=../blas.syms jla_marge_ref_harness.o) && \
!   $FC -o oracle/_ref/jla_marge_ref_harness oracle/_ref/obj/jla_marge_ref_harness.o \
!      $(ls oracle/_ref/obj/*.o | grep -v -e harness -e native -e bench) $OPENBLAS -Wl,-rpath,$OPENBLAS_DIR
!
! and run it inside the dataset's directory (the file names in jla.dataset are
! relative to it):
!
!   (cd DIR/syn37 && ../../oracle/_ref/jla_marge_ref_harness marge.ini lc.txt cases.txt ref.txt)
!
! marge.ini sets use_JLA, JLA_marginalize, the three options and jla_dataset;
! lc.txt is the dataset's light-curve file (zcmb and zhel are its columns 2 and
! 3); cases.txt is the one of the alpha, beta goldens, whose alpha, beta lines
! are skipped.  ref.txt receives per case: -lnL, the grid's points and how many
! of them the reference kept.  The reference prints its own "Error inverting"
! lines on stdout.
module jla_marge_stub
    use settings
    use Calculator_Cosmology
    implicit none

    type, extends(TCosmologyCalculator) :: TStubCalculator
        real(mcp), allocatable :: DA(:)
        integer :: next = 0
    contains
    procedure :: AngularDiameterDistance => Stub_AngularDiameterDistance
    end type TStubCalculator

    contains

    real(mcp) function Stub_AngularDiameterDistance(this, z)
    class(TStubCalculator) :: this
    real(mcp), intent(IN) :: z
    this%next = this%next + 1
    Stub_AngularDiameterDistance = this%DA(this%next)
    end function Stub_AngularDiameterDistance

end module jla_marge_stub

program jla_marge_ref_harness
    use settings
    use GeneralTypes
    use CosmologyTypes
    use CosmoTheory
    use Likelihood_Cosmology
    use JLA
    use jla_marge_stub
    implicit none
    character(len=512) :: ininame, lcname, casefile, outfile
    character(len=4096) :: line
    character(len=64) :: snname
    Type(TSettingIni) :: Ini
    Type(TLikelihoodList) :: List
    Type(TStubCalculator), target :: Stub
    Type(CMBParams) :: CMB
    Type(TCosmoTheoryPredictions) :: Theory
    class(TDataLikelihood), pointer :: Like
    logical :: bad
    integer :: ncase, i, k, u, uo, ul, ios, nz
    real(mcp) :: alpha, beta, v, DataParams(2)
    real(mcp), allocatable :: mu(:), zcmb(:), zhel(:)

    call get_command_argument(1, ininame)
    call get_command_argument(2, lcname)
    call get_command_argument(3, casefile)
    call get_command_argument(4, outfile)
    Feedback = 0
    call Ini%Open(trim(ininame), bad, .false.)
    if (bad) stop 'cannot open the ini'
    call JLALikelihood_Add(List, Ini)
    if (List%Count /= 1) stop 'JLALikelihood_Add added no likelihood'
    allocate(mu(nsn), zcmb(nsn), zhel(nsn), Stub%DA(nsn))
    nz = 0
    open(newunit=ul, file=trim(lcname), status='old')
    do
        read(ul,'(A)',iostat=ios) line
        if (ios /= 0) exit
        if (len_trim(line) == 0) cycle
        if (line(verify(line,' '):verify(line,' ')) == '#') cycle
        nz = nz + 1
        read(line,*) snname, zcmb(nz), zhel(nz)
    end do
    close(ul)
    if (nz /= nsn) stop 'light-curve file and dataset disagree'
    Like => List%Item(1)
    select type (Like)
    class is (JLALikelihood)
        Like%Calculator => Stub
    class default
        stop 'not a JLALikelihood'
    end select
    DataParams = 0
    open(newunit=u, file=trim(casefile), status='old')
    open(newunit=uo, file=trim(outfile), status='replace')
    read(u,*) ncase
    do i = 1, ncase
        read(u,*) alpha, beta
        read(u,*) (mu(k), k=1,nsn)
        do k = 1, nsn
            Stub%DA(k) = 10**(mu(k)/5) / ((1+zhel(k))*(1+zcmb(k)))
        end do
        Stub%next = 0
        select type (Like)
        class is (JLALikelihood)
            v = Like%LogLike(CMB, Theory, DataParams)
        end select
        write(uo,'(ES25.17,2I6)') v, JLA_int_points, count(JLA_marge_grid /= logZero)
    end do
    close(uo)
end program
